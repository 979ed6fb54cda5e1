"""Writes tests/golden/point_cloud_*.npz: the reference's camera point clouds (example/3D/torch/data/*.npz, the inputs
of fit_point_could.py and of the surface SVGP), copied as plain float64 arrays (key `cloud`, (N, 3): x, y, z).

usage: python tests/golden/make_point_cloud_fixtures.py REFERENCE_ROOT"""
import os
import sys

import numpy as np

NAMES = ["distribution", "dustbin_cover", "pan", "white_towelholder", "wood_plate"]


def main(ref_root):
    src = os.path.join(ref_root, "example", "3D", "torch", "data")
    out = os.path.dirname(os.path.abspath(__file__))
    for name in NAMES:
        stem = "point_cloud_distribution" if name == "distribution" else name + "_point_cloud_distribution"
        with np.load(os.path.join(src, stem + ".npz"), allow_pickle=False) as f:
            cloud = np.asarray(f["point_cloud_distribution"], np.float64)
        np.savez_compressed(os.path.join(out, f"point_cloud_{name}.npz"), cloud=cloud)
        print(f"point_cloud_{name}.npz: {cloud.shape}")


if __name__ == "__main__":
    main(sys.argv[1])
