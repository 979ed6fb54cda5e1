"""Headless run of the reference's point-cloud surface fit (example/3D/torch/fit_point_could.py:8-30) on the MI355X path:
for each camera point cloud, SurfaceSVGP with 1000 inducing points, 20 epochs, then the surface on a 100 x 100 grid.
Prints the fit time and the RMS residual at the cloud's own points.

    python examples/point_cloud_surface.py

Data: the arrays of the reference's example/3D/torch/data/*.npz as stored in tests/golden/point_cloud_*.npz."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussian_process_transportation_amd import SurfaceSVGP  # noqa: E402

FILES = ["dustbin_cover", "pan", "white_towelholder", "wood_plate"]

for name in FILES:
    with np.load(os.path.join(ROOT, "tests", "golden", f"point_cloud_{name}.npz")) as f:
        cloud = np.asarray(f["cloud"], np.float64)
    t0 = time.perf_counter()
    gp = SurfaceSVGP(cloud[:, :2], cloud[:, 2].reshape(-1, 1), num_inducing=1000).fit(num_epochs=20)
    t_fit = time.perf_counter() - t0
    x = np.linspace(cloud[:, 0].min(), cloud[:, 0].max(), 100)
    y = np.linspace(cloud[:, 1].min(), cloud[:, 1].max(), 100)
    grid = np.array(np.meshgrid(x, y)).T.reshape(-1, 2)
    new_z, _ = gp.predict(grid, return_std=True)
    surface = np.hstack([grid, new_z.reshape(-1, 1)])
    rms = np.sqrt(np.mean((gp.predict(cloud[:, :2])[:, 0] - cloud[:, 2]) ** 2))
    print(f"{name}: N = {len(cloud)}, fit {t_fit:.2f} s ({len(gp.loss_history_)} steps), surface {surface.shape}, "
          f"RMS residual {rms:.4g} (std z {cloud[:, 2].std():.4g})")
