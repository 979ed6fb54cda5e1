"""apply_transportation() end to end, numpy in to attributes out, with velocities and orientations: fused=False (the three host
calls around the posterior: unchanged code) against fused=True (one gpt_transport_policy call), on the same fitted object in
one session, at one of two sizes per run (so that each gets a time limit of its own):
    small   N = 2500, M = 460, D = 3      (tests/golden/surface_3d.npz: the reference's 3-D demo, the robot demo's quaternions)
    large   N = 8192, M = 500 000, D = 3  (seeded as bench.py seeds its model; the bench's query count)
Next to each: the device-only time of the same posterior launches (gpt_predict_timings on device buffers: mean + J + var + Jvar
at gamma(pos), J at pos).  Warm-up, then the median of --reps alternating runs.  A report; exit status 1 if fused is the slower.
usage: python tools/fused_transport_timing.py --size small|large [--reps 5] [--out FILE (appended)]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import GaussianProcessTransportation, _lib  # noqa: E402


def kernel(c, ls, noise):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    return ConstantKernel(float(c)) * RBF(length_scale=np.atleast_1d(np.asarray(ls, dtype=float)).tolist()) + WhiteKernel(float(noise))


def orientations(M):
    ori = np.load(os.path.join(ROOT, "tests", "golden", "robot_demo_last.npz"))["training_ori"]
    return np.ascontiguousarray(np.resize(ori, (M, 4)))


def problem(size):
    if size == "small":
        g = np.load(os.path.join(ROOT, "tests", "golden", "surface_3d.npz"))
        return (g["source"], g["target"], g["demo"], g["delta"], kernel(g["constant_value"], g["length_scale"], g["noise_level"]))
    N, M = 8192, 500_000
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (N, 3))
    Y = 0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal((N, 3))
    q = np.random.default_rng(1)
    return X, X + Y, q.uniform(-0.1, 1.1, (M, 3)), q.standard_normal((M, 3)), kernel(0.1, [0.1, 0.1, 0.1], 1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=("small", "large"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    import torch
    source, target, demo, delta, k = problem(a.size)
    M = len(demo)
    ori = orientations(M)
    tr = GaussianProcessTransportation(kernel_transport=k, optimizer=None, verbose=False)
    tr.source_distribution, tr.target_distribution = source, target
    tr.fit_transportation()

    def run(fused):
        tr.fused = fused
        tr.training_traj, tr.training_delta, tr.training_ori = demo, delta, ori
        t0 = time.perf_counter()
        tr.apply_transportation()
        return time.perf_counter() - t0, (tr.training_traj, tr.std, tr.training_delta, tr.var_vel_transported, tr.training_ori)
    times = {False: [], True: []}
    res = {}
    for fused in (False, True):
        run(fused)                                             # warm-up: code objects, staging, the variance kernel's plan
    for _ in range(a.reps):
        for fused in (False, True):
            t, res[fused] = run(fused)
            times[fused].append(t)
    diff = [float(np.max(np.abs(x - y)) / np.max(np.abs(y))) for x, y in zip(res[True][:4], res[False][:4])]
    dq = float(np.max(np.minimum(np.linalg.norm(res[True][4] - res[False][4], axis=1), np.linalg.norm(res[True][4] + res[False][4], axis=1))))
    # device-only: the posterior launches on device buffers
    h = tr.method.delta_map._handle
    aff = tr.method.affine_transform
    dev = torch.device("cuda", 0)
    pos = torch.from_numpy(np.ascontiguousarray(demo)).to(dev)
    rot = torch.from_numpy(np.ascontiguousarray(aff.predict(demo))).to(dev)
    mean = torch.empty((M, 3), dtype=torch.float64, device=dev); var = torch.empty(M, dtype=torch.float64, device=dev)
    J = torch.empty((M, 3, 3), dtype=torch.float64, device=dev); Jvar = torch.empty((M, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    h.set_profiling(True)
    device_ms = []
    for _ in range(a.reps + 1):
        h.predict_all_dev(rot.data_ptr(), M, mean.data_ptr(), var.data_ptr(), J.data_ptr(), Jvar.data_ptr())
        t = h.predict_timings()
        at_rot = t["mean_jac_ms"] + t["var_ms"]
        h.predict_all_dev(pos.data_ptr(), M, 0, 0, J.data_ptr())
        device_ms.append(at_rot + h.predict_timings()["mean_jac_ms"])
    h.set_profiling(False)
    device_ms = float(np.median(device_ms[1:]))
    med = {f: 1e3 * float(np.median(times[f])) for f in times}
    N = len(source)
    lines = [f"== {a.size}: N = {N}, M = {M}, D = 3, velocities and orientations, median of {a.reps} (min .. max), ms",
             f"   fused=False (host algebra around three posterior calls): {med[False]:10.3f}  ({1e3 * min(times[False]):.3f} .. {1e3 * max(times[False]):.3f})",
             f"   fused=True  (one gpt_transport_policy call)            : {med[True]:10.3f}  ({1e3 * min(times[True]):.3f} .. {1e3 * max(times[True]):.3f})"
             f"   -> {med[False] / med[True]:.2f} x",
             f"   device-only time of the same posterior launches        : {device_ms:10.3f}",
             f"   fused vs unfused, max-norm relative: traj {diff[0]:.1e}, std {diff[1]:.1e}, vel {diff[2]:.1e}, var_vel {diff[3]:.1e}; "
             f"quaternions (up to sign) {dq:.1e}"]
    for s in lines:
        print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if med[True] <= med[False] else 1


if __name__ == "__main__":
    sys.exit(main())
