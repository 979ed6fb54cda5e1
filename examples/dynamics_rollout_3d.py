"""Headless, seeded roll-out of the 3-D demo's dynamics GP (example/3D/surface_generalization_3D.py:41-49 with the
plot_traj_evolution step of policy_transportation/plot_utils.py:298-309): a C * Matern(nu=1.5) + White GP fitted to the
demonstration's steps, then from a random start inside the demonstration's bounding box, 1000 times
    x <- x + mean(x) - std(x) * grad var(x) / |grad var(x)|
(the step follows the learned velocity and is pulled down the variance towards the demonstration).  grad var is
derivative_of_variance of the Matern model: the analytic derivative of its posterior (matern_derivatives=True).
The loop over the steps runs on the device in one call, GaussianProcess.rollout(..., variance_gain=1); --host runs the loop on
the host instead, two calls per step (predict(return_std=True) and derivative_of_variance), and prints both end distances.

    python examples/dynamics_rollout_3d.py [--steps 1000] [--seed 0] [--host]

Data: the arrays of the reference's example/3D/data/example.npz as stored in tests/golden/surface_3d.npz."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import Matern, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcess as GPR  # noqa: E402


def host_loop(gp, pos, steps):
    """The loop the device call replaces: predict(return_std=True) and derivative_of_variance per step."""
    traj = np.zeros((steps, 3))
    for i in range(steps):
        vel, std = gp.predict(pos, return_std=True)
        grad = gp.derivative_of_variance(pos)[:, 0]                 # (D,) at the one position
        pos = pos + vel.reshape(1, -1) - std[0, 0] * grad / np.linalg.norm(grad)
        traj[i] = pos[0]
    return traj


def main(steps=1000, seed=0, verbose=True, host=False):
    data = np.load(os.path.join(ROOT, "tests", "golden", "surface_3d.npz"))
    X = data["demo"]
    deltaX = np.zeros((len(X), 3))
    deltaX[:-1] = X[1:] - X[:-1]
    gp = GPR(kernel=C(constant_value=np.sqrt(0.1)) * Matern(1 * np.ones(3), nu=1.5) + WhiteKernel(0.01), verbose=False,
             matern_derivatives=True)
    gp.fit(X, deltaX)
    rng = np.random.default_rng(seed)
    pos = rng.uniform(X.min(axis=0), X.max(axis=0)).reshape(1, 3)
    distance = lambda traj: np.min(np.linalg.norm(traj[:, None, :] - X[None, :, :], axis=-1), axis=1)
    t0 = time.perf_counter()
    traj = gp.rollout(pos, steps, variance_gain=1.0)[0, 1:]        # (steps, 3): the points after each step
    t1 = time.perf_counter()
    dist = distance(traj)
    out = dict(traj=traj, distance=dist, seconds=t1 - t0)
    if verbose:
        print(f"dynamics GP kernel: {gp.kernel}")
        print(f"roll-out on the device: {steps} steps in {t1 - t0:.3f} s; distance to the demonstration: start {dist[0]:.3f}, "
              f"end {dist[-1]:.3f}, last 100 steps max {dist[-100:].max():.3f}")
    if host:
        t0 = time.perf_counter()
        traj_h = host_loop(gp, pos, steps)
        t1 = time.perf_counter()
        dist_h = distance(traj_h)
        out.update(traj_host=traj_h, distance_host=dist_h, seconds_host=t1 - t0)
        if verbose:
            print(f"roll-out on the host:   {steps} steps in {t1 - t0:.3f} s; distance to the demonstration: start {dist_h[0]:.3f}, "
                  f"end {dist_h[-1]:.3f}, last 100 steps max {dist_h[-100:].max():.3f}")
            print(f"end distances: device {dist[-1]:.6f}, host {dist_h[-1]:.6f}; largest gap between the two paths "
                  f"{np.max(np.abs(traj - traj_h)):.3e}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="also run the loop on the host, two calls per step, and print both")
    a = ap.parse_args()
    main(a.steps, a.seed, host=a.host)
