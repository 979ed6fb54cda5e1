"""The transported policy at M target-space points, numpy in to numpy out: ONE call (PolicyTransportation.transported_policy:
gpt_pullback_policy) against the composition through the existing public calls — inverse_transport, dynamics.predict,
transport_velocity, each a host round trip — on the same fitted objects in one session.  Shapes:
    2d      N_map = 20,   N_dyn = 400, D = 2   (tests/golden/letterS_2d.npz, the examples' Matern 5/2 dynamics)   M = 1, 400, 10 000
    3d      N_map = 2500, N_dyn = 460, D = 3   (tests/golden/surface_3d.npz, Matern 3/2 dynamics on its demonstration)  M = 1, 460
    large   N_map = 8192, N_dyn = 512, D = 3   (seeded as bench.py seeds its model)                                 M = 100 000
each without and with the variances (return_std), plus the device time of k_pullback_velocity alone (device events around
gpt_pullback_policy_dev with vel and status only, on device buffers).  Warm-up, then the median of --reps alternating runs.  A
report, nothing asserted.
usage: python tools/pullback_timing.py [--shapes 2d 3d large] [--reps 5] [--out FILE (appended)]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportation, _lib  # noqa: E402


def kernel(c, ls, noise, nu=None):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel
    ls = np.atleast_1d(np.asarray(ls, dtype=float)).tolist()
    return ConstantKernel(float(c)) * (RBF(ls) if nu is None else Matern(ls, nu=nu)) + WhiteKernel(float(noise))


def problem(shape):
    """(source, target, transport kernel, demonstration, its velocities, dynamics kernel, query counts)."""
    if shape == "2d":
        g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
        th = np.load(os.path.join(ROOT, "tests", "golden", "matern_2d.npz"))["opt_theta"]
        return (g["source"], g["target"], kernel(g["constant_value"], g["length_scale"], g["noise_level"]), g["demo"], g["delta"],
                kernel(np.exp(th[0]), np.exp(th[1:3]), np.exp(th[3]), 2.5), (1, 400, 10_000))
    if shape == "3d":
        g = np.load(os.path.join(ROOT, "tests", "golden", "surface_3d.npz"))
        return (g["source"], g["target"], kernel(g["constant_value"], g["length_scale"], g["noise_level"]), g["demo"], g["delta"],
                kernel(0.05, [0.5, 0.6, 0.7], 1e-4, 1.5), (1, 460))
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (8192, 3))
    Y = 0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal((8192, 3))
    demo = rng.uniform(0.1, 0.9, (512, 3))
    return X, X + Y, kernel(0.1, [0.1, 0.1, 0.1], 1e-4), demo, 0.1 * np.cos(3 * demo), kernel(0.05, [0.3, 0.3, 0.3], 1e-4, 1.5), (100_000,)


def queries(tr, demo, M):
    """M points of the target scene: the moved demonstration, repeated with a seeded jitter of 1 % of its extent."""
    moved = tr.method.transport(demo, return_std=False)[0]
    rng = np.random.default_rng(M)
    y = np.resize(moved, (M, moved.shape[1]))
    return np.ascontiguousarray(y + 0.01 * (moved.max(axis=0) - moved.min(axis=0)) * rng.standard_normal(y.shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=("2d", "3d", "large"), default=["2d", "3d", "large"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    import torch
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for shape in a.shapes:
        source, target, k_map, demo, delta, k_dyn, counts = problem(shape)
        tr = GaussianProcessTransportation(kernel_transport=k_map, optimizer=None, verbose=False)
        tr.source_distribution, tr.target_distribution = source, target
        tr.fit_transportation()
        dyn = GaussianProcess(kernel=k_dyn, optimizer=None, verbose=False).fit(demo, delta)
        pt, D = tr.method, demo.shape[1]
        aff = pt.affine_transform
        for M in counts:
            y = queries(tr, demo, M)

            def one_call(std):
                t0 = time.perf_counter()
                out = pt.transported_policy(dyn, y, return_std=std)
                return time.perf_counter() - t0, out

            def composition(std):
                t0 = time.perf_counter()
                x = pt.inverse_transport(y)
                if std:
                    f, std_f = dyn.predict(x, return_std=True)
                    v, var_v = pt.transport_velocity(x, f)
                    J_phi = (np.eye(D)[None] + pt.delta_map.derivative(aff.predict(x))) @ aff.rotation_matrix
                    out = (v, np.sqrt(std_f ** 2 * np.sum(J_phi ** 2, axis=2) + var_v))
                else:
                    out = pt.transport_velocity(x, dyn.predict(x), return_var=False)[0]
                return time.perf_counter() - t0, out
            say(f"== {shape}: N_map = {len(source)}, N_dyn = {len(demo)}, D = {D}, M = {M}; median of {a.reps} (min .. max), ms")
            for std in (False, True):
                times = {"one": [], "composed": []}
                res = {}
                for fn in (one_call, composition):
                    fn(std)                                        # warm-up: code objects, staging, the variance kernel's plan
                for _ in range(a.reps):
                    for name, fn in (("composed", composition), ("one", one_call)):
                        t, res[name] = fn(std)
                        times[name].append(t)
                med = {n: 1e3 * float(np.median(t)) for n, t in times.items()}
                v1, v2 = (res["one"][0], res["composed"][0]) if std else (res["one"], res["composed"])
                diff = float(np.max(np.abs(v1 - v2)) / np.max(np.abs(v2)))
                tag = "with variances" if std else "velocities only"
                say(f"   {tag:16s} composition of the public calls: {med['composed']:10.3f}  ({1e3 * min(times['composed']):.3f} .. {1e3 * max(times['composed']):.3f})")
                say(f"   {tag:16s} one call (gpt_pullback_policy) : {med['one']:10.3f}  ({1e3 * min(times['one']):.3f} .. {1e3 * max(times['one']):.3f})"
                    f"   -> {med['composed'] / med['one']:.2f} x; velocities differ by {diff:.1e} (max-norm relative)")
            # device only: k_pullback_velocity on device buffers, device events on the handle's stream
            h, hd = pt.delta_map._handle, dyn._handle
            t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
            yd, R, cs, cd = t(y), t(aff.rotation_matrix), t(aff.S_centroid), t(aff.T_centroid)
            vel = torch.empty((M, D), dtype=torch.float64, device=dev)
            status = torch.empty(M, dtype=torch.int32, device=dev)
            stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            h.set_stream(stream.cuda_stream)
            try:
                ms = []
                for _ in range(a.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        h.pullback_policy_dev(hd, yd.data_ptr(), M, R.data_ptr(), cs.data_ptr(), cd.data_ptr(), float(aff.scale), R.data_ptr(),
                                              vel.data_ptr(), status.data_ptr())
                        e1.record()
                    stream.synchronize()
                    ms.append(e0.elapsed_time(e1))
            finally:
                h.set_stream(0)
            st = np.bincount(status.cpu().numpy(), minlength=4)
            say(f"   device time of k_pullback_velocity alone (events on the stream): {float(np.median(ms[1:])):10.3f}   "
                f"status " + ", ".join(f"{n} {int(c)}" for n, c in zip(_lib.INV_STATUS_NAMES, st)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
