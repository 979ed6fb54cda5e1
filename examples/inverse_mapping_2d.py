"""Headless inverse mapping on the 2-D letter-S: the reference's inverse-mapping example
(example/2D/surface_generalization_heteroschedastic _inverse_mapping.py:88-127) fits a SECOND transport with source and
target swapped and walks a 100 x 100 grid of target-space points through it in a Python loop.  Here the fitted map itself is
inverted: the grid is pulled back to the source space by GaussianProcessTransportation.inverse_transport, one launch.

    python examples/inverse_mapping_2d.py

Data, kernel and hyper-parameters: tests/golden/letterS_2d.npz (the reference's example/2D/data/example.npz, resampled, and
the theta its optimizer found).  The map folds near the demonstration (det(I + J_psi) <= 0 at some of its points), so not
every target point has one preimage; the printout says how many queries ended in which state."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C  # noqa: E402

from gaussian_process_transportation_amd import GaussianProcessTransportation as Transport  # noqa: E402
from gaussian_process_transportation_amd._lib import INV_CONVERGED, INV_STATUS_NAMES  # noqa: E402


def main(verbose=True, n_grid=100):
    g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
    kernel = C(float(g["constant_value"])) * RBF(g["length_scale"].tolist()) + WhiteKernel(float(g["noise_level"]))
    transport = Transport(kernel_transport=kernel, optimizer=None, verbose=False)
    transport.source_distribution, transport.target_distribution = g["source"], g["target"]
    transport.training_traj = g["demo"]
    transport.fit_transportation(do_scale=False, do_rotation=True)
    transport.apply_transportation()
    moved = transport.training_traj
    lo, hi = moved.min(axis=0), moved.max(axis=0)
    pad = 0.3 * (hi - lo)
    xg, yg = np.meshgrid(np.linspace(lo[0] - pad[0], hi[0] + pad[0], n_grid), np.linspace(lo[1] - pad[1], hi[1] + pad[1], n_grid))
    grid = np.column_stack([xg.ravel(), yg.ravel()])
    back, info = transport.inverse_transport(grid, return_info=True)
    solved = info["status"] == INV_CONVERGED
    # the pulled-back points, pushed forward again, land on the grid
    again = transport.method.transport(back[solved], return_std=False)[0]
    miss = float(np.max(np.linalg.norm(again - grid[solved], axis=1))) if solved.any() else float("nan")
    hist = np.bincount(info["passes"])
    if verbose:
        print(f"{len(grid)} target-space points pulled back through the letter-S map")
        print("status: " + ", ".join(f"{name} {int(np.sum(info['status'] == code))}" for code, name in enumerate(INV_STATUS_NAMES)))
        print("passes: " + ", ".join(f"{p}: {n}" for p, n in enumerate(hist) if n))
        print(f"det(I + J_psi) <= 0 at {np.mean(info['det'][solved] <= 0):.1%} of the solutions (a fold: that preimage is one of several)")
        print(f"forward map of the solutions misses the grid by at most {miss:.2e}")
    return dict(grid=grid, back=back, info=info, round_trip=miss, pass_histogram=hist)


if __name__ == "__main__":
    main()
