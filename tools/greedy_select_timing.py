"""Timing of the greedy subset selection (gpt_select_greedy) on one GPU -> profiles/greedy_select_timing.txt.

Per (N, m), D = 3, RBF: wall time of the whole call (allocation, upload, the m insertions, download), median of --repeat
runs after one warm-up; the bytes the column kernel streams from the pool factor, 8 N j per insertion = 4 N m (m - 1) in
all; and that traffic over the time, against the 6.3 TB/s a streaming copy reaches on this part.
--one N M runs a single call (to be traced: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/greedy_select_timing.py --one N M); --trace-csv FILE N M then summarises DIR's *_kernel_trace.csv: kernel time of the
column and reduction launches, the time of one insertion at j = m (mean of the last 32 column launches) and the traffic over
the kernel time alone.
--baseline: the only way to do the same job without the entry point — GaussianProcess(optimizer=None).fit(subset) +
predict(pool, return_std=True) per insertion — at N = 20 000, m = 512 from the 51 initial points, against the new path on
the same input in the same session.

The (20 000, 8192) row is the one size whose insertions beyond j = 4096 read the pivot row's tail from global memory.
--isa (no GPU): compiles csrc/gpt_select.hip to gfx950 assembly and reports, per sel_column instantiation, VGPRs, LDS,
private segment (scratch), SGPR spills (v_writelane / v_readlane into a VGPR, no memory) and how many of those lane
operations sit in basic blocks that issue 16-byte loads of the pool factor (the column loops).
--reference REFERENCE_ROOT (no GPU): the reference class itself (gaussian_process_al.py, fixed-bound kernel) on the CPU at
N = 2000, m = 120.
Every mode prints its lines; --out FILE writes them, --append adds them to FILE instead.  profiles/greedy_select_timing.txt
is, in this order (F = the profile, one GPU session for the first four):
    python tools/greedy_select_timing.py --baseline --out F
    for (N, M) in (20000, 4096), (200000, 4096), (1000000, 1024), (20000, 8192):
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/greedy_select_timing.py --one N M
        python tools/greedy_select_timing.py --trace-csv DIR/.../*_kernel_trace.csv N M --out F --append
    python tools/greedy_select_timing.py --reference REFERENCE_ROOT --out F --append
    python tools/greedy_select_timing.py --isa --out F --append

usage: python tools/greedy_select_timing.py [--quick] [--baseline] [--repeat 3] [--out FILE] [--append]"""
import argparse
import csv
import contextlib
import importlib.util
import io
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gaussian_process_transportation_amd import GaussianProcess, _lib  # noqa: E402  (no library is loaded at import)

COPY_TBS = 6.3
C, NOISE, ALPHA, LS = 0.1, 1e-4, 1e-10, 0.2


def pool(N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, 3))
    return X, 0.05 * np.sin(4 * X)


def timed(X, m, initial, repeat):
    ts = []
    for r in range(repeat + 1):
        t = time.perf_counter()
        out = _lib.select_greedy(X, np.full(3, LS), C, NOISE, ALPHA, m, initial=initial, residual=False)
        if r:
            ts.append(time.perf_counter() - t)
    return statistics.median(ts), out


def baseline(X, Y, m, initial):
    """fit + predict per insertion with the package's public class (what the parent commit offers)."""
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as CK
    kern = CK(C, "fixed") * RBF(np.full(3, LS), "fixed") + WhiteKernel(NOISE, "fixed")
    gp = GaussianProcess(kern, alpha=ALPHA, optimizer=None, verbose=False)
    sel = list(initial)
    alive = np.ones(len(X), bool)
    alive[initial] = False
    t = time.perf_counter()
    while len(sel) < m:
        gp.fit(X[sel], Y[sel])
        _, std = gp.predict(X, return_std=True)
        p = int(np.argmax(np.where(alive, std[:, 0], -np.inf)))
        sel.append(p)
        alive[p] = False
    return time.perf_counter() - t, np.array(sel)


def summarise_trace(path, N, m):
    rows = list(csv.DictReader(open(path)))
    col = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "sel_column" in r["Kernel_Name"])
    nxt = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "sel_next" in r["Kernel_Name"]]
    t_col, t_nxt = sum(e - b for b, e in col) * 1e-9, sum(e - b for b, e in nxt) * 1e-9
    span = (col[-1][1] - col[0][0]) * 1e-9
    last = sum(e - b for b, e in col[-32:]) / len(col[-32:]) * 1e-6
    tb = 4.0 * N * m * (m - 1) / 1e12
    return (f"kernel trace, N = {N}, m = {m}: {len(col)} column launches {t_col:.4f} s, {len(nxt)} reductions {t_nxt:.4f} s "
            f"({t_nxt / max(len(nxt), 1) * 1e6:.1f} us each), first to last kernel {span:.4f} s; one insertion at j = m "
            f"{last:.3f} ms = {8e-9 * N * m / last:.2f} TB/s; {tb:.3f} TB over the column kernels' time {tb / t_col:.2f} TB/s "
            f"= {tb / t_col / COPY_TBS:.1%} of the {COPY_TBS} TB/s copy rate")


def isa_report():
    src = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc", "gpt_select.hip")
    asm = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                          "-Wno-unused-value", "-fno-gpu-rdc", "--cuda-device-only", "-S", src, "-o", "-"], check=True,
                         capture_output=True, text=True).stdout
    lines = ["ISA (hipcc -S, gfx950):"]
    for lpr in (8, 16, 64):
        name = re.search(rf"^(_ZN\w*sel_columnILi{lpr}E\w*):", asm, flags=re.M).group(1)
        body = asm[asm.index("\n" + name + ":"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        meta = asm[asm.index(f".name:           {name}"):]          # the metadata record: the spill counts follow the name
        num = lambda key, text: int(re.search(key + r"\s*:?\s+(\d+)", text).group(1))
        blocks = re.split(r"^\.LBB\d+_\d+:", body, flags=re.M)
        lane = lambda b: len(re.findall(r"v_(?:read|write)lane_b32", b))
        in_loops = sum(lane(b) for b in blocks if "global_load_dwordx4" in b)
        lines.append(f"  sel_column<{lpr}>: {num(r'amdhsa_next_free_vgpr', body)} VGPRs, {num(r'amdhsa_group_segment_fixed_size', body)} bytes of LDS, "
                     f"private segment {num(r'amdhsa_private_segment_fixed_size', body)} (scratch instructions {len(re.findall('scratch_', body))}), "
                     f"SGPR spills {num(r'sgpr_spill_count', meta)} / VGPR spills {num(r'vgpr_spill_count', meta)}; {lane(body)} lane operations for them, "
                     f"{in_loops} in blocks that load the pool factor")
    return lines


def reference_cpu(ref_root):
    os.environ.setdefault("MPLBACKEND", "Agg")
    spec = importlib.util.spec_from_file_location("reference_gaussian_process_al",
                                                  os.path.join(ref_root, "policy_transportation", "models", "gaussian_process_al.py"))
    al = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(al)
    al.tqdm = lambda it: it
    import sklearn
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as CK
    N, m = 2000, 120
    X, Y = pool(N)
    g = al.GaussianProcess(CK(C, "fixed") * RBF(np.full(3, LS), "fixed") + WhiteKernel(NOISE, "fixed"), alpha=ALPHA, n_samples_max=m)
    np.random.seed(0)
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        g.fit(X, Y)
    return [f"reference class on a CPU (gaussian_process_al.py, fixed-bound kernel, scikit-learn {sklearn.__version__}): "
            f"{time.perf_counter() - t:.1f} s at N = {N}, m = {m}"]


def emit(a, lines):
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa", action="store_true")
    ap.add_argument("--reference", metavar="REFERENCE_ROOT")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--one", nargs=2, type=int, metavar=("N", "M"))
    ap.add_argument("--trace-csv", nargs=3, metavar=("FILE", "N", "M"))
    ap.add_argument("--quick", action="store_true", help="N = 20 000 only")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_csv:
        return emit(a, [summarise_trace(a.trace_csv[0], int(a.trace_csv[1]), int(a.trace_csv[2]))])
    if a.isa:
        return emit(a, isa_report())
    if a.reference:
        return emit(a, reference_cpu(a.reference))
    _lib.require_gpu()
    if a.one:
        N, m = a.one
        X, _ = pool(N)
        t = time.perf_counter()
        _lib.select_greedy(X, np.full(3, LS), C, NOISE, ALPHA, m, initial=np.random.default_rng(1).choice(N, int(0.1 * m), replace=False),
                           residual=False)
        print(f"N = {N}, m = {m}: {time.perf_counter() - t:.3f} s")
        return
    lines = [f"greedy subset selection, D = 3, RBF (l = {LS}, c = {C}, noise = {NOISE}), fp64; median of {a.repeat} after a warm-up",
             f"{'N':>9} {'m':>5} {'total s':>9} {'TB streamed':>12} {'TB/s':>7} {'of 6.3 TB/s copy':>17}"]
    sizes = [(20000, 512), (20000, 2048), (20000, 4096)]
    if not a.quick:
        sizes += [(200000, 512), (200000, 2048), (200000, 4096), (1000000, 1024), (20000, 8192)]
    for N, m in sizes:
        X, _ = pool(N)
        initial = np.random.default_rng(1).choice(N, int(0.1 * m), replace=False)
        t_full, _ = timed(X, m, initial, a.repeat)
        tb = 4.0 * N * m * (m - 1) / 1e12
        lines.append(f"{N:>9} {m:>5} {t_full:>9.3f} {tb:>12.3f} {tb / t_full:>7.2f} "
                     f"{tb / t_full / COPY_TBS:>16.1%}")
        print(lines[-1], flush=True)
    if a.baseline:
        N, m = 20000, 512
        X, Y = pool(N)
        initial = np.random.default_rng(1).choice(N, int(0.1 * m), replace=False)
        baseline(X, Y, len(initial) + 8, initial)                       # warm-up
        tb_, sel_b = zip(*[baseline(X, Y, m, initial) for _ in range(a.repeat)])
        t_new, out = timed(X, m, initial, a.repeat)
        same = int(np.sum(out[0] == sel_b[0]))
        lines.append(f"baseline, N = {N}, m = {m} from {len(initial)}: GaussianProcess(optimizer=None).fit + predict(return_std) per "
                     f"insertion {statistics.median(tb_):.3f} s; gpt_select_greedy {t_new:.4f} s; ratio {statistics.median(tb_) / t_new:.0f}x "
                     f"({same} of {m} indices identical)")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
