"""Many frame pairs at once: the shape of the reference's multi-frame ablation
(example/comparisons/multi_reference_frames/ablation_study_gpt.py:29-64 over models/model_gpt.py:74-83) on synthetic data —
10-point source / target distributions per frame pair, a demonstration of about 200 points, one source sent to 8 targets,
hyper-parameters optimised per pair (5 restarts).  The batch class fits and transports every pair together; the loop below
it does what the reference does, one GaussianProcessTransportation per pair.  Prints both wall times.
--optimizer device_bfgs runs the batch's hyper-parameter search on the device (one workgroup per run) in place of scipy's
L-BFGS-B threads; the loop keeps scipy's.

usage: python examples/multi_frame_batch.py [n_pairs] [--optimizer fmin_l_bfgs_b|device_bfgs]      (needs an MI355X)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frame_pairs(n_pairs=8, n_points=10, n_traj=200, seed=0):
    """One source frame cloud and demonstration, sent to n_pairs target clouds (rotated, shifted, locally bent)."""
    rng = np.random.default_rng(seed)
    source = rng.uniform(-1, 1, (n_points, 2))
    s = np.linspace(0, 1, n_traj)
    traj = np.column_stack([1.6 * s - 0.8, 0.5 * np.sin(2 * np.pi * s)])
    vel = np.gradient(traj, axis=0)
    pairs = []
    for _ in range(n_pairs):
        ang = rng.uniform(-0.6, 0.6)
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        target = source @ R.T + rng.uniform(-0.5, 0.5, 2) + 0.08 * np.sin(3 * source[:, ::-1]) + 0.005 * rng.standard_normal(source.shape)
        pairs.append((source, target, traj, vel))
    return pairs


def kernel():
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel as C, WhiteKernel
    return C(0.1) * RBF(length_scale=[1.0, 1.0]) + WhiteKernel(0.0001)


def run_batch(pairs, seed=0, optimizer="fmin_l_bfgs_b"):
    from gaussian_process_transportation_amd import GaussianProcessTransportationBatch
    np.random.seed(seed)
    tb = GaussianProcessTransportationBatch(kernel_transport=kernel(), optimizer=optimizer)
    tb.source_distributions, tb.target_distributions, tb.training_trajs, tb.training_deltas = map(list, zip(*pairs))
    tb.fit_transportations()
    tb.apply_transportations()
    return tb


def run_loop(pairs, seed=0):
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    np.random.seed(seed)
    out = []
    for source, target, traj, vel in pairs:
        tr = GaussianProcessTransportation(kernel_transport=kernel(), verbose=False)
        tr.source_distribution, tr.target_distribution, tr.training_traj, tr.training_delta = source, target, traj, vel
        tr.fit_transportation()
        tr.apply_transportation()
        out.append(tr)
    return out


def main():
    args = sys.argv[1:]
    optimizer = "fmin_l_bfgs_b"
    if "--optimizer" in args:
        optimizer = args.pop(args.index("--optimizer") + 1)
        args.remove("--optimizer")
    n_pairs = int(args[0]) if args else 8
    pairs = frame_pairs(n_pairs)
    run_batch(pairs[:2], optimizer=optimizer)             # first-call costs (library load, LDS opt-in) outside the timing
    t0 = time.perf_counter()
    tb = run_batch(pairs, optimizer=optimizer)
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    loop = run_loop(pairs)
    t_loop = time.perf_counter() - t0
    worst = max(float(np.max(np.abs(tb.training_trajs[b] - loop[b].training_traj))) for b in range(n_pairs))
    st = tb.regressor.optimizer_stats_
    search = (f"{st['calls']} batched objective calls" if optimizer == "fmin_l_bfgs_b" else
              f"{optimizer}: {st['runs']} runs, {st['launches']} launches, {st['evaluations']} evaluations")
    print(f"{n_pairs} frame pairs, optimiser on: batch {t_batch:.3f} s ({search}), "
          f"per-pair loop {t_loop:.3f} s; largest difference between the moved trajectories {worst:.2e}")


if __name__ == "__main__":
    main()
