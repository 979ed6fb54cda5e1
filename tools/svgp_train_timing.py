"""Times one optimiser step of the SVGP variational training: the fused HIP path (gpt_svgp_train: every step enqueued
back to back, one call for the whole schedule) against eager torch autograd + torch.optim.Adam of the same fp64
restatement (tests/svgp_elbo_restatement.py) on the same GPU, in the same process.  Shapes (Z, T, D, B) of the issue;
N = 2500 training points (the reference's 3-D example).  Writes the table to --out (default profiles/svgp_train_timing.txt).

    python tools/svgp_train_timing.py [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import _lib  # noqa: E402
from gaussian_process_transportation_amd.svgp_exact import svgp_schedule  # noqa: E402
from tests import svgp_elbo_restatement as sr  # noqa: E402

SHAPES = [(100, 3, 3, 10), (200, 2, 2, 10), (1000, 1, 2, 10)]
N = 2500
REF_STEPS = 2500          # the reference example: 10 epochs x 250 minibatches


def problem(Zn, T, D):
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([0.3 * np.sin(3 * X.sum(1) / np.sqrt(D) + t) for t in range(T)], 1)
    return X, Y, sr.init_params(X, Y, rng.choice(N, Zn))


def fused(X, Y, p, B, steps, reps=3):
    np.random.seed(0)
    idx, bb = svgp_schedule(N, int(np.ceil(steps * B / N)), B)
    bb = bb[:steps + 1]
    _lib.svgp_train(X, Y, {k: v.copy() for k, v in p.items()}, idx, bb)          # warm-up (module load, allocation)
    best = np.inf
    for _ in range(reps):
        q = {k: v.copy() for k, v in p.items()}
        t0 = time.perf_counter()
        _lib.svgp_train(X, Y, q, idx, bb)
        best = min(best, time.perf_counter() - t0)
    return best / steps * 1e6


def eager(X, Y, p, B, steps, warm=3):
    dev = "cuda"
    tp = sr.to_torch(p, requires_grad=True, device=dev)
    Xt, Yt = torch.tensor(X, device=dev), torch.tensor(Y, device=dev)
    opt = torch.optim.Adam([tp[k] for k in sr.PARAM_NAMES], lr=0.01)
    rng = np.random.default_rng(1)
    rows = [torch.tensor(rng.choice(N, B, replace=False), device=dev) for _ in range(warm + steps)]

    def step(r):
        opt.zero_grad()
        sr.loss(tp, Xt[r], Yt[r], N).backward()
        opt.step()
    for r in rows[:warm]:
        step(r)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in rows[warm:]:
        step(r)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgp_train_timing.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    lines = [f"SVGP variational training, one Adam step on the negative ELBO, fp64, N = {N}; {torch.cuda.get_device_name(0)}",
             "fused = gpt_svgp_train (2 launches per step, whole schedule in one call, best of 3 wall-clock runs incl. copies);",
             "eager = torch autograd + torch.optim.Adam on tests/svgp_elbo_restatement.py, same GPU, same process.",
             f"{'Z':>5} {'T':>3} {'D':>3} {'B':>4} | {'fused us/step':>13} {'eager us/step':>13} {'ratio':>7} | "
             f"{'fused 2500 steps s':>18} {'eager 2500 steps s':>18}"]
    for Zn, T, D, B in SHAPES:
        X, Y, p = problem(Zn, T, D)
        steps_f = 500 if Zn <= 200 else 20
        steps_e = 50 if Zn <= 200 else 5
        f = fused(X, Y, p, B, steps_f)
        print(f"Z={Zn} T={T} D={D} B={B}: fused {f:.1f} us/step", flush=True)
        e = eager(X, Y, p, B, steps_e)
        print(f"Z={Zn} T={T} D={D} B={B}: eager {e:.1f} us/step", flush=True)
        lines.append(f"{Zn:>5} {T:>3} {D:>3} {B:>4} | {f:>13.1f} {e:>13.1f} {e / f:>7.1f} | {f * REF_STEPS * 1e-6:>18.3f} "
                     f"{e * REF_STEPS * 1e-6:>18.3f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
