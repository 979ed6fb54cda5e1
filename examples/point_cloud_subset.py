"""Greedy subset selection on a camera point cloud: a dense resampling of a committed cloud (60 000 points) is reduced to
600 by ActiveLearningGaussianProcess — the reference's gaussian_process_al.GaussianProcess — and the exact GP is fitted on
the subset.  Prints the largest posterior variance over the pool before and after the selection.

usage: python examples/point_cloud_subset.py [cloud name, default pan]"""
import os
import sys

import numpy as np
from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import _lib  # noqa: E402
from gaussian_process_transportation_amd.gaussian_process_al import GaussianProcess  # noqa: E402


def main(name="pan", n_pool=60000, n_samples_max=600):
    with np.load(os.path.join(ROOT, "tests", "golden", f"point_cloud_{name}.npz"), allow_pickle=False) as f:
        cloud = np.asarray(f["cloud"], np.float64)
    cloud = (cloud - cloud.mean(0)) / np.abs(cloud - cloud.mean(0)).max()
    rng = np.random.default_rng(0)
    # dense resampling: every pool point is a cloud point moved by a fraction of the cloud's spacing
    pool = cloud[rng.integers(0, len(cloud), n_pool)] + 0.02 * rng.standard_normal((n_pool, 3))
    targets = 0.05 * np.sin(4 * pool)                       # a smooth displacement field to transport
    c, ls, noise, alpha = 0.1, np.full(3, 0.25), 1e-4, 1e-10
    kernel = C(c, "fixed") * RBF(ls, "fixed") + WhiteKernel(noise, "fixed")
    np.random.seed(0)
    gp = GaussianProcess(kernel, alpha=alpha, n_samples_max=n_samples_max, verbose=False).fit(pool, targets)
    n_initial = n_samples_max - gp.selection_variance_.size
    # the residual variance over the pool after the initial random subset alone, and after the whole selection
    _, _, before = _lib.select_greedy(pool, ls, c, noise, alpha, n_initial, initial=gp.selected_indices_[:n_initial])
    _, _, after = _lib.select_greedy(pool, ls, c, noise, alpha, n_samples_max, initial=gp.selected_indices_)
    mean, std = gp.predict(pool, return_std=True)
    print(f"pool {pool.shape}, selected {gp.X.shape[0]} ({n_initial} random + {gp.selection_variance_.size} greedy)")
    print(f"largest posterior variance over the pool: {before.max():.3e} after the random subset, {after.max():.3e} after the selection "
          f"(prior {c + noise:.3e}, noise floor {noise:.1e})")
    print(f"fit on the subset: max |mean - target| over the pool {np.abs(mean - targets).max():.2e}, largest predicted std {std.max():.2e}")


if __name__ == "__main__":
    main(*sys.argv[1:2])
