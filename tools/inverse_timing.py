"""The fused inverse (gpt_inverse_map: damped Newton, one wave per query, one launch) against THE SAME iteration driven from the
host over the existing forward path, in one session, at three shapes:
    letter-S        N = 20,   D = 2, M = 400    (tests/golden/letterS_2d.npz: the golden trajectory)
    surface_3d      N = 2500, D = 3, M = 10^4   (tests/golden/surface_3d.npz: a 25 x 20 x 20 grid over the trajectory's box)
    bench model     N = 8192, D = 3, M = 10^5   (seeded as bench.py: targets y = x + mean(x) of uniform x)
The host loop is what can be written without the kernel: per pass ONE predict_all(mean, J) call on the queries still running
(one launch where predict + derivative would make two, and finished queries dropped: the strongest form of it), the D x D
solves and the accept / reject step in numpy.  Both sides take numpy arrays and return numpy arrays.  Outputs are compared.
Also: device time of the fused launch per query-pass (device buffers, stream synchronised) next to k_mean_jac's time per query
at the same N (gpt_predict_timings).  A report; the one condition is that the fused call is the faster of the two everywhere.
usage: python tools/inverse_timing.py [--reps 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import _lib  # noqa: E402
from gaussian_process_transportation_amd.affine_transform import AffineTransform  # noqa: E402


def host_loop(h, y, rtol=1e-10, max_passes=64):
    """The iteration of gpt_inverse_map (include/gpt_hip.h) with every pass a predict_all call."""
    M, D = y.shape
    eye = np.eye(D)[None]

    def evaluate(z, yy):
        out = h.predict_all(z, mean=True, J=True)
        return z + out["mean"] - yy, eye + out["J"]
    z = y.copy()
    r, A = evaluate(z, y)
    rho = np.linalg.norm(r, axis=1)
    tol = rtol * (1.0 + np.linalg.norm(y, axis=1))
    t = np.ones(M); passes = np.ones(M, dtype=np.int32); status = np.full(M, -1, dtype=np.int32)
    while True:
        status[(status < 0) & (rho <= tol)] = _lib.INV_CONVERGED
        status[(status < 0) & (passes == max_passes)] = _lib.INV_MAX_PASSES
        det = np.linalg.det(A)
        status[(status < 0) & (np.abs(det) <= 2.0 ** -40 * np.sqrt(np.sum(A * A, axis=(1, 2))) ** D)] = _lib.INV_SINGULAR
        idx = np.flatnonzero(status < 0)
        if idx.size == 0:
            break
        zn = z[idx] - t[idx, None] * np.linalg.solve(A[idx], r[idx][:, :, None])[:, :, 0]
        rn, An = evaluate(zn, y[idx])
        passes[idx] += 1
        rhon = np.linalg.norm(rn, axis=1)
        ok = rhon < rho[idx]
        acc, rej = idx[ok], idx[~ok]
        z[acc], r[acc], A[acc], rho[acc] = zn[ok], rn[ok], An[ok], rhon[ok]
        t[acc] = np.minimum(1.0, 2.0 * t[acc])
        t[rej] *= 0.5
        status[rej[t[rej] < 2.0 ** -20]] = _lib.INV_STALLED
    return z, {"status": status, "passes": passes, "residual": rho, "det": np.linalg.det(A)}


def transport_model(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    aff = AffineTransform(verbose=False).fit(g["source"], g["target"])
    src = aff.predict(g["source"])
    h = _lib.Handle(0)
    h.fit(src, g["target"] - src, g["length_scale"], float(g["constant_value"]), float(g["noise_level"]), 1e-10)
    return h, g


def shapes():
    h, g = transport_model("letterS_2d")
    yield "letter-S", h, np.ascontiguousarray(g["traj"])
    h, g = transport_model("surface_3d")
    lo, hi = g["traj"].min(axis=0), g["traj"].max(axis=0)
    ax = [np.linspace(lo[d], hi[d], n) for d, n in enumerate((25, 20, 20))]
    yield "surface_3d", h, np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    N, M = 8192, 100_000
    rng = np.random.default_rng(0)                       # (oracle.synthetic_problem's draws, as bench.py seeds its model)
    X = rng.uniform(0, 1, (N, 3))
    Y = 0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal((N, 3))
    Xq = np.random.default_rng(1).uniform(-0.1, 1.1, (M, 3))
    h = _lib.Handle(0)
    h.fit(X, Y, np.array([0.1, 0.1, 0.1]), 0.1, 1e-4, 1e-10)
    yield "bench model", h, Xq + h.predict_all(Xq, mean=True)["mean"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    import torch
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    all_faster = True
    for name, h, y in shapes():
        N, D, _, _ = h.info()
        M = len(y)
        z, info = h.inverse_map(y)                                       # warm-up of both sides (code objects, staging)
        zh, ih = host_loop(h, y)
        fused, loop = [], []
        for _ in range(a.reps):                                          # alternating, best of reps
            t0 = time.perf_counter(); z, info = h.inverse_map(y); fused.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); zh, ih = host_loop(h, y); loop.append(time.perf_counter() - t0)
        # device time of the launch alone
        yd = torch.from_numpy(y).to(dev)
        zd = torch.empty_like(yd); st = torch.empty(M, dtype=torch.int32, device=dev); ps = torch.empty(M, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        kern = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            h.inverse_map_dev(yd.data_ptr(), M, zd.data_ptr(), st.data_ptr(), passes_ptr=ps.data_ptr())
            h.synchronize()
            kern.append(time.perf_counter() - t0)
        kern = min(kern[1:])
        # k_mean_jac at the same N and M: time per query
        mean = torch.empty((M, D), dtype=torch.float64, device=dev); J = torch.empty((M, D, D), dtype=torch.float64, device=dev)
        h.set_profiling(True)
        mj = []
        for _ in range(a.reps + 1):
            h.predict_all_dev(yd.data_ptr(), M, mean.data_ptr(), 0, J.data_ptr())
            mj.append(h.predict_timings()["mean_jac_ms"])
        h.set_profiling(False)
        mj = min(mj[1:])
        same = info["status"] == ih["status"]
        both = (info["status"] == _lib.INV_CONVERGED) & (ih["status"] == _lib.INV_CONVERGED)
        dz = float(np.max(np.linalg.norm(z - zh, axis=1)[both])) if both.any() else float("nan")
        qp = int(info["passes"].sum())
        hist = np.bincount(info["passes"])
        say(f"== {name}: N = {N}, D = {D}, M = {M}")
        say("   status (fused): " + ", ".join(f"{n} {int(np.sum(info['status'] == c))}" for c, n in enumerate(_lib.INV_STATUS_NAMES))
            + f"; same status as the host loop at {int(same.sum())} of {M}; max |z_fused - z_loop| where both converged {dz:.2e}")
        say("   passes (fused): " + ", ".join(f"{p}: {n}" for p, n in enumerate(hist) if n) + f"  (host loop: {int(ih['passes'].max())} predict_all calls)")
        say(f"   fused call, numpy in / out : {1e3 * min(fused):9.3f} ms (best of {a.reps}; median {1e3 * float(np.median(fused)):.3f})")
        say(f"   host-driven loop           : {1e3 * min(loop):9.3f} ms (best of {a.reps}; median {1e3 * float(np.median(loop)):.3f})"
            f"   -> fused is {min(loop) / min(fused):.1f} x faster")
        say(f"   fused launch on device buffers: {1e3 * kern:.3f} ms = {1e9 * kern / qp:.1f} ns per query-pass ({qp} query-passes); "
            f"k_mean_jac (mean + J, {M} queries): {mj:.3f} ms = {1e6 * mj / M:.1f} ns per query")
        all_faster &= min(fused) < min(loop)
        h.close()
    say("fused faster than the host-driven loop at every shape: " + ("yes" if all_faster else "NO"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all_faster else 1


if __name__ == "__main__":
    sys.exit(main())
