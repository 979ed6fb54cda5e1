"""Headless transported policy through TWO transports on the 2-D letter-S: the reference's obstacle example
(example/2D/surface_generalization_with_obstacle.py:142-200) moves the demonstration from the old surface to the new one and
then, with a second transport fitted in the new scene, bends it round an obstacle; it then refits a GP on the twice-moved
demonstration.  Here the dynamics fitted ONCE in the source scene is pulled back through both maps in one device call
(TransportChain.transported_policy): for every point y of a 100 x 100 grid of the final scene, x = (Phi_1 o Phi_0)^-1(y) and
v(y) = J_Phi_1 J_Phi_0 f(x), with its std — the dynamics' own uncertainty and each map's Jacobian variance carried through the
maps after it.

    python examples/obstacle_chain_2d.py

Data: tests/golden/letterS_2d.npz (the reference's example/2D/data/example.npz, resampled, and the theta its optimizer found
for the first transport).  The obstacle: three rings of 12 points round a point of the moved demonstration, radii 3, 9 and 20,
pushed outwards by 2, 0.5 and 0, so the second map opens a hole there and fades out away from it.  The first map folds near
the demonstration, so not every grid point has one preimage: the printout says how many queries ended in which state at
which stage.  Last lines: on the twice-moved demonstration, started at the demonstration, every stage takes one pass and the
pulled-back field is the forward-transported velocity."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportation as Transport, TransportChain  # noqa: E402
from gaussian_process_transportation_amd._lib import INV_CONVERGED, INV_STATUS_NAMES  # noqa: E402


def rings(centre, push=(2.0, 0.5, 0.0), radii=(3.0, 9.0, 20.0), n=12):
    ang = 2 * np.pi * np.arange(n) / n
    u = np.column_stack([np.cos(ang), np.sin(ang)])
    return (np.concatenate([centre + r * u for r in radii]), np.concatenate([centre + (r + p) * u for r, p in zip(radii, push)]))


def main(verbose=True, n_grid=100):
    np.random.seed(0)
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
    twice, twice_vel, _, stds = chain.transport(g["demo"], vel=g["delta"])
    lo, hi = twice.min(axis=0) - 5, twice.max(axis=0) + 5
    xg, yg = np.meshgrid(np.linspace(lo[0], hi[0], n_grid), np.linspace(lo[1], hi[1], n_grid))
    grid = np.column_stack([xg.ravel(), yg.ravel()])
    vel, std, info = chain.transported_policy(dynamics, grid, return_std=True, return_info=True)
    solved = info["status"] == INV_CONVERGED
    on_demo, on_info = chain.transported_policy(dynamics, twice, x0=g["demo"], return_info=True)
    f_demo = dynamics.predict(g["demo"])
    pushed = chain.transport(g["demo"], vel=f_demo)[1]
    miss = np.linalg.norm(on_demo - pushed, axis=1)
    if verbose:
        print(f"{len(grid)} points of the final scene: the source dynamics pulled back through the letter-S map and the obstacle map")
        for k in (1, 0):
            print(f"stage {k}: " + ", ".join(f"{name} {int(np.sum(info['stage_status'][k] == code))}" for code, name in enumerate(INV_STATUS_NAMES))
                  + f"; passes <= {int(info['stage_passes'][k].max())}")
        print(f"the demonstration is moved by up to {np.linalg.norm(twice - moved, axis=1).max():.2f} by the obstacle map "
              f"(std of the two maps on it: median {np.median(stds[0]):.3f}, {np.median(stds[1]):.3f})")
        speed = np.linalg.norm(vel[solved], axis=1)
        print(f"speed on the grid: median {np.median(speed):.3f}, largest {speed.max():.3f} (far from the demonstration the dynamics is 0); "
              f"std of it median {np.median(std[solved]):.3f}")
        print(f"on the twice-moved demonstration: passes per stage {on_info['stage_passes'].max(axis=1).tolist()}, preimage off the "
              f"demonstration by <= {np.linalg.norm(on_info['x'] - g['demo'], axis=1).max():.1e}, velocity off the forward-transported one by <= {miss.max():.1e}")
    return dict(grid=grid, vel=vel, std=std, info=info, miss=miss)


if __name__ == "__main__":
    main()
