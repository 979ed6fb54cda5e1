"""The transported policy through TWO transports at M target-space points, numpy in to numpy out: ONE call
(TransportChain.transported_policy: gpt_pullback_chain) against the three-call cascade through the existing public methods —
inverse_transport on the outer map, transported_policy on the inner map, transport_velocity on the outer map again — on the
same fitted objects in one session.  Shapes:
    2d      letter-S (N = 20) then the obstacle rings (N = 36), dynamics on the demonstration (N = 400), D = 2   M = 1, 10 000 (the 100 x 100 grid)
    large   N_map = 8192 twice, N_dyn = 512, D = 3 (seeded as tools/pullback_timing.py seeds its model)            M = 100 000
each without and with the std (the cascade's std: the inner call's variances pushed through the outer Jacobian, plus the outer
map's own transport_velocity variance).  Warm-up, then the median of --reps runs, the two paths interleaved.  A report; the one
condition it checks is printed per line: the chain call is not slower than the cascade by more than the spread (max - min) of
the cascade's own runs.
usage: python tools/chain_timing.py [--shapes 2d large] [--reps 5] [--out FILE (appended)]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportation, TransportChain, _lib  # noqa: E402


def kernel(c, ls, noise, nu=None):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, WhiteKernel
    ls = np.atleast_1d(np.asarray(ls, dtype=float)).tolist()
    return ConstantKernel(float(c)) * (RBF(ls) if nu is None else Matern(ls, nu=nu)) + WhiteKernel(float(noise))


def rings(centre, push=(2.0, 0.5, 0.0), radii=(3.0, 9.0, 20.0), n=12):
    ang = 2 * np.pi * np.arange(n) / n
    u = np.column_stack([np.cos(ang), np.sin(ang)])
    return (np.concatenate([centre + r * u for r in radii]), np.concatenate([centre + (r + p) * u for r, p in zip(radii, push)]))


def fit(source, target, k):
    tr = GaussianProcessTransportation(kernel_transport=k, optimizer=None, verbose=False)
    tr.source_distribution, tr.target_distribution = source, target
    tr.fit_transportation()
    return tr


def problem(shape):
    """(the two fitted transports, the fitted dynamics, {label: queries})."""
    if shape == "2d":
        g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
        tr0 = fit(g["source"], g["target"], kernel(g["constant_value"], g["length_scale"], g["noise_level"]))
        moved = tr0.method.transport(g["demo"], return_std=False)[0]
        tr1 = fit(*rings(moved[200]), kernel(4.0, [6.0, 6.0], 1e-3))
        dyn = GaussianProcess(kernel=kernel(0.3, [1.5, 2.5], 0.01), optimizer=None, verbose=False).fit(g["demo"], g["delta"])
        twice = tr1.method.transport(moved, return_std=False)[0]
        lo, hi = twice.min(axis=0) - 5, twice.max(axis=0) + 5
        xg, yg = np.meshgrid(np.linspace(lo[0], hi[0], 100), np.linspace(lo[1], hi[1], 100))
        return [tr0, tr1], dyn, {"M = 1": np.ascontiguousarray(twice[200:201]),
                                 "M = 10000 (100 x 100 grid)": np.ascontiguousarray(np.column_stack([xg.ravel(), yg.ravel()]))}
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (8192, 3))
    tr0 = fit(X, X + 0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal(X.shape), kernel(0.1, [0.1, 0.1, 0.1], 1e-4))
    X1 = rng.uniform(0, 1, (8192, 3))
    tr1 = fit(X1, X1 + 0.04 * np.cos(3 * X1) + 0.01 * rng.standard_normal(X1.shape), kernel(0.1, [0.12, 0.12, 0.12], 1e-4))
    demo = rng.uniform(0.1, 0.9, (512, 3))
    dyn = GaussianProcess(kernel=kernel(0.05, [0.3, 0.3, 0.3], 1e-4, 1.5), optimizer=None, verbose=False).fit(demo, 0.1 * np.cos(3 * demo))
    twice = TransportChain([tr0, tr1], verbose=False).transport(demo)[0]
    y = np.resize(twice, (100_000, 3)) + 0.005 * np.random.default_rng(1).standard_normal((100_000, 3))
    return [tr0, tr1], dyn, {"M = 100000": np.ascontiguousarray(y)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=("2d", "large"), default=["2d", "large"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for shape in a.shapes:
        trs, dyn, sets = problem(shape)
        chain = TransportChain(trs, verbose=False)
        inner, outer = trs[0].method, trs[1].method
        D = chain.n_features
        for label, y in sets.items():
            def one_call(std):
                t0 = time.perf_counter()
                out = chain.transported_policy(dyn, y, return_std=std)
                return time.perf_counter() - t0, out

            def cascade(std):
                t0 = time.perf_counter()
                mid = outer.inverse_transport(y)
                if std:
                    v, s = inner.transported_policy(dyn, mid, return_std=True)
                    w, var_w = outer.transport_velocity(mid, v)
                    aff = outer.affine_transform
                    B = (np.eye(D)[None] + outer.delta_map.derivative(aff.predict(mid))) @ aff.rotation_matrix
                    out = (w, np.sqrt(np.einsum("mij,mj->mi", B ** 2, s ** 2) + var_w))
                else:
                    out = outer.transport_velocity(mid, inner.transported_policy(dyn, mid), return_var=False)[0]
                return time.perf_counter() - t0, out
            say(f"== {shape}: N_map = {len(trs[0].source_distribution)} + {len(trs[1].source_distribution)}, N_dyn = {len(dyn.X)}, D = {D}, "
                f"{label}; median of {a.reps} (min .. max), ms")
            for std in (False, True):
                times, res = {"one": [], "cascade": []}, {}
                for fn in (one_call, cascade):
                    fn(std)                                            # warm-up: code objects, staging, the variance kernels' plans
                for _ in range(a.reps):
                    for name, fn in (("cascade", cascade), ("one", one_call)):
                        t, res[name] = fn(std)
                        times[name].append(t)
                med = {n: 1e3 * float(np.median(t)) for n, t in times.items()}
                spread = 1e3 * (max(times["cascade"]) - min(times["cascade"]))
                v1, v2 = (res["one"][0], res["cascade"][0]) if std else (res["one"], res["cascade"])
                ok = np.isfinite(v2).all(axis=1)
                diff = float(np.max(np.abs(v1[ok] - v2[ok])) / np.max(np.abs(v2[ok])))
                tag = "with std" if std else "velocities only"
                say(f"   {tag:16s} cascade of three public calls  : {med['cascade']:10.3f}  ({1e3 * min(times['cascade']):.3f} .. {1e3 * max(times['cascade']):.3f})")
                say(f"   {tag:16s} one call (gpt_pullback_chain)  : {med['one']:10.3f}  ({1e3 * min(times['one']):.3f} .. {1e3 * max(times['one']):.3f})"
                    f"   -> {med['cascade'] / med['one']:.2f} x; not slower by more than the cascade's spread ({spread:.3f}): "
                    f"{'yes' if med['one'] <= med['cascade'] + spread else 'NO'}; velocities differ by {diff:.1e} (max-norm relative)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
