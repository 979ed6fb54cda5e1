"""Matern 5/2 against RBF for the derivative paths: k_var time (profiling events of the handle) and the end-to-end rate of
gpt_predict_all (numpy in, numpy out), modes J+Jvar (J, Jacobian variance) and dvar (d var / dx), fp64 and fp32.
N = 8192 sources in 3-D, M = 200 000 queries by default.  A report, not a gate.
usage: python tools/matern_deriv_timing.py [--n 8192] [--m 200000] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--m", type=int, default=200_000)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
_lib.require_gpu()
rng = np.random.default_rng(0)
X = rng.uniform(0, 1, (a.n, 3))
Y = 0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal((a.n, 3))
Xq = np.random.default_rng(1).uniform(-0.1, 1.1, (a.m, 3))
MODES = {"J+Jvar": dict(J=True, Jvar=True), "dvar": dict(dvar=True)}
rows = []
for dtype, dname in ((_lib.GPT_F64, "fp64"), (_lib.GPT_F32, "fp32")):
    xq = Xq.astype(np.float32) if dtype == _lib.GPT_F32 else Xq
    for kt, kname in ((0, "RBF"), (3, "Matern52")):
        h = _lib.Handle(0)
        h.set_dtype(dtype)
        h.set_matern_derivatives(True)
        h.fit(X, Y, np.array([0.1, 0.1, 0.1]), 0.1, 1e-4, 1e-10, kt)
        for mode, flags in MODES.items():
            h.predict_all(xq[:4096], **flags)                      # warm-up: plan, scratch, code objects
            h.predict_all(xq, **flags)
            h.set_profiling(True)
            kvar, wall = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                h.predict_all(xq, **flags)
                wall.append(time.perf_counter() - t0)
                kvar.append(h.predict_timings()["var_ms"])
            h.set_profiling(False)
            rows.append(dict(dtype=dname, kernel=kname, mode=mode, N=a.n, M=a.m, kvar_ms=min(kvar), e2e_ms=1e3 * min(wall),
                             e2e_kq_per_s=a.m / min(wall) / 1e3))
        h.close()
for r in rows:
    base = next(b for b in rows if b["dtype"] == r["dtype"] and b["mode"] == r["mode"] and b["kernel"] == "RBF")
    r["kvar_vs_rbf"] = r["kvar_ms"] / base["kvar_ms"]
    r["e2e_vs_rbf"] = r["e2e_ms"] / base["e2e_ms"]
    print(f"{r['dtype']} {r['kernel']:9s} {r['mode']:7s} N={r['N']} M={r['M']}: k_var {r['kvar_ms']:8.2f} ms ({r['kvar_vs_rbf']:.3f} x RBF) | "
          f"end to end {r['e2e_ms']:8.1f} ms = {r['e2e_kq_per_s']:7.1f} k q/s ({r['e2e_vs_rbf']:.3f} x RBF)")
print(json.dumps(rows))
