"""Times the point-cloud surface SVGP (svgp_surface.py): one optimiser step of gpt_svgp_surface_train (every step enqueued
back to back, one call for the whole schedule) against eager torch autograd + torch.optim.Adam of the same fp64
restatement (tests/svgp_surface_restatement.py) on the same GPU, in the same process; the reference's whole flow
(fit_point_could.py: N = 495, Z = 1000, 20 epochs); prediction on its 100 x 100 grid; the RMS residual that flow leaves on
each of the five committed clouds.  Warm-up, synchronised, best of 3.
Writes the table to --out (default profiles/svgp_surface_timing.txt).

    python tools/svgp_surface_timing.py [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import SurfaceSVGP, _lib  # noqa: E402
from gaussian_process_transportation_amd.svgp_exact import svgp_schedule  # noqa: E402
from tests import svgp_surface_restatement as ss  # noqa: E402

CLOUDS = ["distribution", "dustbin_cover", "pan", "white_towelholder", "wood_plate"]
SHAPES = [(1000, 1, 2, 10), (1000, 3, 2, 10), (200, 2, 2, 10), (100, 3, 3, 10)]
N = 500


def problem(Zn, T, D):
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([0.3 * np.sin(3 * X.sum(1) / np.sqrt(D) + t) for t in range(T)], 1)
    return X, Y, ss.init_params(X, Y, rng.choice(N, Zn))


def best_of(fn, reps=3):
    fn()                                          # warm-up (module load, allocation, kernel attributes)
    best = np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def device_step(X, Y, p, B, steps):
    np.random.seed(0)
    idx, bb = svgp_schedule(N, int(np.ceil(steps * B / N)), B)
    bb = bb[:steps + 1]
    return best_of(lambda: _lib.svgp_surface_train(X, Y, {k: v.copy() for k, v in p.items()}, idx, bb)) / steps * 1e6


def eager_step(X, Y, p, B, steps, warm=3):
    dev = "cuda"
    tp = ss.to_torch(p, requires_grad=True, device=dev)
    Xt, Yt = torch.tensor(X, device=dev), torch.tensor(Y, device=dev)
    opt = torch.optim.Adam([tp[k] for k in ss.PARAM_NAMES], lr=0.01)
    rng = np.random.default_rng(1)
    rows = [torch.tensor(rng.choice(N, B, replace=False), device=dev) for _ in range(warm + steps)]

    def step(r):
        opt.zero_grad()
        ss.loss(tp, Xt[r], Yt[r], N).backward()
        opt.step()
    for r in rows[:warm]:
        step(r)
    best = np.inf
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in rows[warm:]:
            step(r)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgp_surface_timing.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    lines = [f"Surface SVGP (per-task length-scale), one Adam step on the negative ELBO, fp64, N = {N}; {torch.cuda.get_device_name(0)}",
             "device = gpt_svgp_surface_train (whole schedule in one call, best of 3 wall-clock runs incl. copies);",
             "eager = torch autograd + torch.optim.Adam on tests/svgp_surface_restatement.py, same GPU, same process, best of 3.",
             f"{'Z':>5} {'T':>3} {'D':>3} {'B':>4} | {'device us/step':>14} {'eager us/step':>13} {'eager/device':>12}"]
    for Zn, T, D, B in SHAPES:
        X, Y, p = problem(Zn, T, D)
        d = device_step(X, Y, p, B, 100)
        e = eager_step(X, Y, p, B, 20)
        lines.append(f"{Zn:>5} {T:>3} {D:>3} {B:>4} | {d:>14.1f} {e:>13.1f} {e / d:>12.2f}")
        print(lines[-1], flush=True)
    with np.load(os.path.join(ROOT, "tests", "golden", "point_cloud_distribution.npz")) as f:
        cloud = np.asarray(f["cloud"], np.float64)
    models = []

    def flow():
        np.random.seed(0)
        models.append(SurfaceSVGP(cloud[:, :2], cloud[:, 2:], num_inducing=1000).fit(num_epochs=20))
    t_fit = best_of(flow)
    model = models[-1]
    xs = np.linspace(cloud[:, 0].min(), cloud[:, 0].max(), 100)
    ys = np.linspace(cloud[:, 1].min(), cloud[:, 1].max(), 100)
    grid = np.array(np.meshgrid(xs, ys)).T.reshape(-1, 2)
    t_pred = best_of(lambda: model.predict(grid, return_std=True))
    t_jac = best_of(lambda: model.derivative(grid))
    steps = len(model.loss_history_)
    lines.append(f"reference flow (fit_point_could.py): N = {len(cloud)}, Z = 1000, 20 epochs = {steps} steps: {t_fit:.3f} s "
                 f"({t_fit / steps * 1e3:.3f} ms/step incl. setup and copies)")
    lines.append(f"prediction on the 100 x 100 grid (M = 10^4, Z = 1000): mean + std {t_pred * 1e3:.2f} ms, J {t_jac * 1e3:.2f} ms")
    lines.append("fit quality of that flow (np.random.seed(0)): RMS residual of predict(cloud[:, :2]) / std(z); "
                 "constant mean(z) = 1, untrained model (predicts 0) in brackets")
    for name in CLOUDS:
        with np.load(os.path.join(ROOT, "tests", "golden", f"point_cloud_{name}.npz")) as f:
            c3 = np.asarray(f["cloud"], np.float64)
        np.random.seed(0)
        gp = SurfaceSVGP(c3[:, :2], c3[:, 2:], num_inducing=1000).fit(num_epochs=20)
        sd = c3[:, 2].std()
        rms = np.sqrt(np.mean((gp.predict(c3[:, :2])[:, 0] - c3[:, 2]) ** 2))
        lines.append(f"  {name:<18} N = {len(c3):>3}: {rms / sd:.4f}  ({np.sqrt(np.mean(c3[:, 2] ** 2)) / sd:.3f})")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
