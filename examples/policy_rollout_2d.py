"""Headless rollout of the transported policy on the 2-D letter-S with an obstacle: the scene of examples/obstacle_chain_2d.py
(the demonstration moved to the new surface by the letter-S transport, then bent round an obstacle by a second transport fitted
in the new scene), and the streamlines of the policy that the source dynamics becomes there.  The reference integrates such a
policy on the host, 1000 steps of pos += vel (plot_traj_evolution); here a 10 x 10 grid of starts is integrated in ONE device call
(TransportChain.rollout): every step inverts both maps at the current point, started at the preimage of the step before,
evaluates the dynamics there and pushes it forward.

    python examples/policy_rollout_2d.py

Data: tests/golden/letterS_2d.npz.  The first map folds near the demonstration, so a path can reach a point with no single
preimage; it ends there, and the printout says how many paths ended early and with which status.  Only the mean policy is
integrated (the reference's pull down the variance gradient, rollout(..., variance_gain=g), is examples/dynamics_rollout_3d.py's subject)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportation as Transport, TransportChain  # noqa: E402
from gaussian_process_transportation_amd._lib import INV_STATUS_NAMES  # noqa: E402


def rings(centre, push=(2.0, 0.5, 0.0), radii=(3.0, 9.0, 20.0), n=12):
    ang = 2 * np.pi * np.arange(n) / n
    u = np.column_stack([np.cos(ang), np.sin(ang)])
    return (np.concatenate([centre + r * u for r in radii]), np.concatenate([centre + (r + p) * u for r, p in zip(radii, push)]))


def main(verbose=True, n_grid=10, n_steps=200, dt=1.0):
    g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
    dynamics = GaussianProcess(kernel=C(0.3) * RBF([1.5, 2.5]) + WhiteKernel(0.01), optimizer=None, verbose=False).fit(g["demo"], g["delta"])
    first = Transport(kernel_transport=C(float(g["constant_value"])) * RBF(g["length_scale"].tolist()) + WhiteKernel(float(g["noise_level"])),
                      optimizer=None, verbose=False)
    first.source_distribution, first.target_distribution = g["source"], g["target"]
    first.fit_transportation()
    moved = first.method.transport(g["demo"], return_std=False)[0]
    second = Transport(kernel_transport=C(4.0) * RBF([6.0, 6.0]) + WhiteKernel(1e-3), optimizer=None, verbose=False)
    second.source_distribution, second.target_distribution = rings(moved[200])
    second.fit_transportation()
    chain = TransportChain([first, second], verbose=False)
    twice = chain.transport(g["demo"])[0]
    lo, hi = twice.min(axis=0), twice.max(axis=0)
    xg, yg = np.meshgrid(np.linspace(lo[0], hi[0], n_grid), np.linspace(lo[1], hi[1], n_grid))
    starts = np.column_stack([xg.ravel(), yg.ravel()])
    path, info = chain.rollout(dynamics, starts, n_steps, dt=dt, return_info=True)
    done = info["steps_done"]
    ends = path[np.arange(len(path)), done]                              # the last point every path recorded
    # the robot's own path: from the start of the twice-moved demonstration, its preimage the start of the demonstration
    own, own_info = chain.rollout(dynamics, twice[:1], len(twice) - 1, dt=dt, x0=g["demo"][:1], return_info=True)
    n_own = int(own_info["steps_done"][0])
    off = np.linalg.norm(own[0, :n_own + 1] - twice[:n_own + 1], axis=1)
    if verbose:
        print(f"{len(starts)} starts on a {n_grid} x {n_grid} grid over the twice-moved demonstration, {n_steps} steps of dt = {dt} in one device call")
        print(f"steps done: min {int(done.min())}, median {int(np.median(done))}, max {int(done.max())}; complete paths: {int(np.sum(done == n_steps))}")
        print("status of the last step evaluated: " + ", ".join(f"{name} {int(np.sum(info['status'] == code))}" for code, name in enumerate(INV_STATUS_NAMES)))
        print(f"end points: spread (std per axis) {np.std(ends, axis=0).round(2).tolist()} against {np.std(starts, axis=0).round(2).tolist()} of the starts; "
              f"median distance to the end of the demonstration {np.median(np.linalg.norm(ends - twice[-1], axis=1)):.2f}")
        print(f"from the demonstration's own start: {n_own} steps done, off the twice-moved demonstration by <= {off.max():.2f} "
              f"(it is {np.linalg.norm(twice[-1] - twice[0]):.1f} from end to end)")
    return dict(starts=starts, path=path, info=info, ends=ends, own=own, own_info=own_info)


if __name__ == "__main__":
    main()
