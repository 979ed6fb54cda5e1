"""Headless, seeded: which paths does the letter-S dynamics GP consider plausible from the demonstration's start?  A
C * RBF + White GP is fitted to the demonstration's steps (tests/golden/letterS_2d.npz: demo -> delta, 400 points).  The mean
path follows its posterior mean.  A SAMPLED path follows ONE function drawn from the posterior: the value drawn at a step is
conditioned on what the same function was drawn to be at the path's own earlier points, because the errors of a GP at
neighbouring points are almost perfectly correlated and the path keeps revisiting the same region.  32 such paths from the start of
the demonstration, beside the mean path, in one device call (GaussianProcess.rollout_samples); printed: the spread of the sampled
paths per step, beside what independent noise of the marginal standard deviation per step would give.

--host also runs the loop on the host from calls that were there before: per path and step predict(points so far,
return_cov=True), np.linalg.cholesky and the draw from the factor's last row, with the same normals.  It is also the way beyond
_lib.ROLLOUT_SAMPLED_MAX_T steps or _lib.ROLLOUT_STAB_MAX_N training points.

    python examples/sampled_rollout_2d.py [--steps 100] [--samples 32] [--seed 0] [--host]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcess as GPR  # noqa: E402


def host_loop(gp, start, normals, dt=1.0):
    """The loop the device call replaces, one path: normals (T,D).  The covariance of predict(return_cov=True) carries the noise
    level on its diagonal, which is the nugget rollout_samples takes by default."""
    T, D = normals.shape
    path = np.full((T + 1, D), np.nan)
    path[0] = start
    for t in range(T):
        mean, cov = gp.predict(np.ascontiguousarray(path[:t + 1]), return_cov=True)
        g = np.linalg.cholesky(cov[..., 0] if cov.ndim == 3 else cov)[t]
        path[t + 1] = path[t] + dt * (mean[t] + g @ normals[:t + 1])
    return path


def main(steps=100, samples=32, seed=0, verbose=True, host=False):
    data = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
    X, deltaX = data["demo"], data["delta"]
    gp = GPR(kernel=C(constant_value=0.3) * RBF([1.5, 2.5]) + WhiteKernel(0.01), optimizer=None, verbose=False)
    gp.fit(X, deltaX)
    start = np.ascontiguousarray(X[:1])
    normals = np.random.RandomState(seed).standard_normal((1, samples, steps, 2))
    t0 = time.perf_counter()
    paths, info = gp.rollout_samples(start, steps, n_samples=samples, normals=normals, return_info=True)
    t1 = time.perf_counter()
    mean_path = gp.rollout(start, steps)[0]
    paths = paths[0]                                                 # (samples, steps + 1, 2)
    spread = np.sqrt(np.mean(np.sum((paths - mean_path[None]) ** 2, axis=-1), axis=0))       # rms distance from the mean path
    naive = np.sqrt(np.cumsum(2 * np.mean(info["pvar"][0], axis=0)))                          # independent noise per step, D = 2, dt = 1
    out = dict(paths=paths, mean_path=mean_path, spread=spread, naive=naive[-1], seconds=t1 - t0, info=info)
    if verbose:
        print(f"dynamics GP kernel: {gp.kernel}")
        print(f"{samples} sampled paths of {steps} steps on the device in {t1 - t0:.3f} s; complete: {int(np.sum(info['steps_done'] == steps))}")
        print("step   rms distance of the sampled paths from the mean path   (independent noise per step would give)")
        for t in sorted(set(list(range(0, steps + 1, max(1, steps // 10))) + [steps])):
            print(f"{t:4d}   {spread[t]:10.4f}   ({0.0 if t == 0 else naive[t - 1]:.4f})")
    if host:
        t0 = time.perf_counter()
        host_paths = np.stack([host_loop(gp, start[0], normals[0, j]) for j in range(samples)])
        t1 = time.perf_counter()
        out.update(paths_host=host_paths, seconds_host=t1 - t0)
        if verbose:
            print(f"the same on the host, predict(return_cov=True) + cholesky per path and step: {t1 - t0:.3f} s; largest gap between the two "
                  f"sets of paths {np.nanmax(np.abs(host_paths - paths)):.3e} (the dynamics amplifies rounding)")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="also run the loop on the host, one predict(return_cov=True) per path and step")
    a = ap.parse_args()
    main(a.steps, a.samples, a.seed, host=a.host)
