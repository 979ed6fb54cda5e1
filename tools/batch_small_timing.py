"""Timing of the batch of small models -> profiles/batch_small_models.txt.

  python tools/batch_small_timing.py --resources        (CPU only: hipcc -save-temps, the factor kernel's resource summary)
  timeout 900 python tools/batch_small_timing.py --gpu  (on an MI355X: the measurements)
  Each run replaces its own section of the file and keeps the others (the hand-written "# old against new" among them);
  --out FILE names another file than the profile.

Objective: the median of 20 runs of one gpt_batch_lml_objective at B = 64, n = 20, D = 2, O = 2 against 64 sequential
Handle.lml_objective calls on one handle; the batched call must take no longer than 8 of the sequential calls (one launch
and one small copy each way against at least eight dependent launches per call: a worse ratio means the batch does not run
as one launch).  End to end: examples/multi_frame_batch.py's workload at 8 and 160 pairs — batch class, per-pair loop of
GaussianProcessTransportation, scikit-learn on the host CPU.

Device search (optimizer='device_bfgs') -> profiles/batch_device_search.txt:
  python tools/batch_small_timing.py --device-search --resources      (CPU only: bat_optimize's resource summary)
  timeout 900 python tools/batch_small_timing.py --device-search --gpu  (on an MI355X: the end-to-end rows at 8 and 160 pairs
      against the coalesced scipy path, interleaved, median of 5, and one launch of 64 evaluations of an n = 128 model)
  python tools/batch_small_timing.py --device-search --once 160       (one search after a warm-up: run it under
      rocprofv3 --kernel-trace --stats for the duration of every bat_optimize launch)"""
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "batch_small_models.txt")
CSRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc")


def resources(unit, kernel):
    """The compiler's resource report of one kernel's instantiations in a unit of csrc (CPU only)."""
    lines = []
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-value", "-fno-gpu-rdc",
                        "-save-temps", "-c", os.path.join(CSRC, unit + ".hip"), "-o", os.path.join(d, unit + ".o")], check=True, cwd=d,
                       stderr=subprocess.DEVNULL)
        asm = open([os.path.join(d, f) for f in os.listdir(d) if f.endswith(".s") and "amdgcn" in f][0]).read()
    for m in re.finditer(r"\.amdhsa_kernel (\S*" + kernel + r"\S*)(.*?)\.end_amdhsa_kernel", asm, flags=re.S):
        def field(k):
            r = re.search(r"\.amdhsa_" + k + r"\s+(\S+)", m.group(2))
            return r.group(1) if r else "?"
        nmax, kt, obj = re.search(kernel + r"ILi(\d+)ELi(\d)E(?:Lb(\d))?", m.group(1)).groups()
        dyn = (int(nmax) * (int(nmax) + 1) + int(nmax) * 16 + int(nmax)) * 8
        name = f"{kernel}<NMAX={nmax}, KT={kt}" + (f", OBJ={obj}>" if obj else ">")
        lines.append(f"{name}: VGPRs {field('next_free_vgpr')}, SGPRs {field('next_free_sgpr')}, "
                     f"static LDS {field('group_segment_fixed_size')} B, dynamic LDS (computed) {dyn} B, scratch {field('private_segment_fixed_size')} B")
    return lines


def gpu():
    from examples.multi_frame_batch import frame_pairs, kernel, run_batch, run_loop
    from gaussian_process_transportation_amd import _lib
    lines = []
    rng = np.random.default_rng(0)
    B = 64
    Xs = [rng.uniform(0, 1, (20, 2)) for _ in range(B)]
    Ys = [np.sin(3 * x) + 0.01 * rng.standard_normal(x.shape) for x in Xs]
    X, Y, nb = _lib.batch_pack(Xs, Ys)
    ls, c, noise = np.full((B, 2), 0.3), np.ones(B), np.full(B, 1e-3)
    h = _lib.Handle(0)
    for _ in range(3):
        _lib.batch_lml_objective_packed(X, Y, nb, ls, c, noise, 1e-10)
        h.lml_objective(Xs[0], Ys[0], ls[0], 1.0, 1e-3, 1e-10)
    tb, ts = [], []
    for _ in range(20):
        t0 = time.perf_counter()
        _lib.batch_lml_objective_packed(X, Y, nb, ls, c, noise, 1e-10)
        tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for b in range(B):
            h.lml_objective(Xs[b], Ys[b], ls[b], 1.0, 1e-3, 1e-10)
        ts.append(time.perf_counter() - t0)
    tb, ts = float(np.median(tb)), float(np.median(ts))
    ratio = tb / (ts / B)
    lines.append(f"objective, B = 64, n = 20, D = 2, O = 2 (median of 20): batched call {1e6 * tb:.0f} us; 64 sequential Handle.lml_objective "
                 f"calls {1e6 * ts:.0f} us ({1e6 * ts / B:.0f} us each); the batched call costs {ratio:.2f} sequential calls "
                 f"(requirement: <= 8) -> {'met' if ratio <= 8 else 'NOT MET'}")
    from sklearn.gaussian_process import GaussianProcessRegressor
    from gaussian_process_transportation_amd.affine_transform import AffineTransform
    run_batch(frame_pairs(2))
    for n_pairs in (8, 160):
        pairs = frame_pairs(n_pairs)
        t0 = time.perf_counter()
        res = run_batch(pairs)
        t_batch = time.perf_counter() - t0
        t0 = time.perf_counter()
        run_loop(pairs)
        t_loop = time.perf_counter() - t0
        np.random.seed(0)
        t0 = time.perf_counter()
        for source, target, traj, vel in pairs:        # the reference's fit + predict on the CPU (the derivative algebra left out)
            aff = AffineTransform(verbose=False).fit(source, target)
            src = aff.predict(source)
            gp = GaussianProcessRegressor(kernel=kernel(), alpha=1e-10, n_restarts_optimizer=5).fit(src, target - src)
            gp.predict(aff.predict(traj), return_std=True)
        t_cpu = time.perf_counter() - t0
        lines.append(f"end to end, {n_pairs} pairs (n = 10, M = 200, optimiser on, 5 restarts): batch class {t_batch:.3f} s "
                     f"({res.regressor.optimizer_stats_['calls']} batched objective calls for {res.regressor.optimizer_stats_['runs']} runs), "
                     f"loop of GaussianProcessTransportation {t_loop:.3f} s, scikit-learn on the CPU (fit + predict with std only) {t_cpu:.3f} s")
    return lines, ratio


SEARCH_OUT = os.path.join(ROOT, "profiles", "batch_device_search.txt")


def search_once(n_pairs):
    """One device search of the end-to-end workload after a warm-up: the program a kernel trace is taken of."""
    from examples.multi_frame_batch import frame_pairs, run_batch
    run_batch(frame_pairs(2), optimizer="device_bfgs")
    res = run_batch(frame_pairs(n_pairs), optimizer="device_bfgs")
    print(n_pairs, "pairs:", res.regressor.optimizer_stats_)


def search_gpu():
    """Device search against the coalesced scipy path, interleaved, median of 5; one launch of 64 evaluations of an n = 128 model."""
    from examples.multi_frame_batch import frame_pairs, run_batch
    from gaussian_process_transportation_amd import _lib
    lines = []
    for optimizer in ("fmin_l_bfgs_b", "device_bfgs"):
        run_batch(frame_pairs(2), optimizer=optimizer)
    for n_pairs in (8, 160):
        pairs = frame_pairs(n_pairs)
        times = {"fmin_l_bfgs_b": [], "device_bfgs": []}
        stats = {}
        for _ in range(5):
            for optimizer in times:
                t0 = time.perf_counter()
                res = run_batch(pairs, optimizer=optimizer)
                times[optimizer].append(time.perf_counter() - t0)
                stats[optimizer] = dict(res.regressor.optimizer_stats_)
        a, b = np.array(times["fmin_l_bfgs_b"]), np.array(times["device_bfgs"])
        lines.append(f"end to end, {n_pairs} pairs (n = 10, M = 200, 5 restarts; interleaved, median of 5 [min .. max]): "
                     f"scipy path {np.median(a):.3f} s [{a.min():.3f} .. {a.max():.3f}] ({stats['fmin_l_bfgs_b']['calls']} batched objective calls, "
                     f"{stats['fmin_l_bfgs_b']['runs']} runs); device search {np.median(b):.3f} s [{b.min():.3f} .. {b.max():.3f}] "
                     f"({stats['device_bfgs']['runs']} runs, {stats['device_bfgs']['launches']} launches, "
                     f"{stats['device_bfgs']['evaluations']} evaluations)")
    # a launch is bounded by evals_per_launch = 64 evaluations of an n = 128 model: one call whose only launch spends them
    rng = np.random.default_rng(0)
    for D, n_ls, O in ((2, 2, 2), (15, 15, 16)):
        X = rng.uniform(0, 1, (128, D))
        Y = np.sin(3 * X @ rng.standard_normal((D, O))) + 0.05 * rng.standard_normal((128, O))
        nb = np.array([0, 128], dtype=np.int64)
        bounds = np.log(np.array([[1e-2, 1e2]] + [[5e-2, 2e1]] * n_ls + [[1e-4, 1e-1]]))
        theta0 = bounds.mean(axis=1)[None]
        t = {}
        for cap in (1, 64):
            best, evals = np.inf, None
            for _ in range(7):
                t0 = time.perf_counter()
                out = _lib.batch_optimize_packed(X, Y, nb, n_ls, np.zeros(1, dtype=np.int32), theta0, bounds, 1e-10, max_evals=cap,
                                                 evals_per_launch=64)
                best = min(best, time.perf_counter() - t0)
                evals = int(out[3][0])
            t[cap] = (best, evals)
        per = (t[64][0] - t[1][0]) / max(1, t[64][1] - t[1][1])
        lines.append(f"one launch, one run, n = 128, D = {D}, n_ls = {n_ls}, O = {O} (host clock around the whole call, best of 7): "
                     f"{t[1][1]} evaluation {1e6 * t[1][0]:.0f} us, {t[64][1]} evaluations {1e6 * t[64][0]:.0f} us "
                     f"-> {1e6 * per:.0f} us per evaluation; a launch at evals_per_launch = 64 lasts {1e3 * 64 * per:.2f} ms")
    return lines


def search_main():
    """--device-search --resources | --gpu | --once N: the sections of profiles/batch_device_search.txt, or the traced program."""
    global HEADS
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else SEARCH_OUT
    HEADS = {"resources": "# resources of bat_optimize (hipcc --offload-arch=gfx950 -save-temps, as for bat_factor in batch_small_models.txt)",
             "measurements": "# measurements on an MI355X (tools/batch_small_timing.py --device-search --gpu)",
             "old_new": OLD_NEW_HEAD,
             "notes": "# notes"}
    if "--once" in sys.argv:
        search_once(int(sys.argv[sys.argv.index("--once") + 1]))
    if "--resources" in sys.argv:
        write_section(out, "resources", sorted(resources("gpt_batch_opt", "bat_optimize")))
    if "--gpu" in sys.argv:
        lines = search_gpu()
        write_section(out, "measurements", lines)
        print("\n".join(lines))


OLD_NEW_HEAD = "# old against new (written by hand from an A/B of two builds; this tool keeps the section as it is)"
HEADS = {"resources": "# resources of bat_factor (hipcc --offload-arch=gfx950 -save-temps: VGPRs, SGPRs, static LDS and scratch from the "
                      "compiler's kernel descriptor; the dynamic LDS is what the launch asks for, computed here as BatCfg::factor_lds does)",
         "measurements": "# measurements on an MI355X (tools/batch_small_timing.py --gpu)",
         "old_new": OLD_NEW_HEAD}


def write_section(path, name, lines):
    """Replaces one section of the profile (a HEADS line and what follows it up to the next one) and keeps the other."""
    sections = {k: [] for k in HEADS}
    current = None
    if os.path.exists(path):
        for line in open(path).read().splitlines():
            hit = [k for k, h in HEADS.items() if line.split(" (")[0] == h.split(" (")[0]]
            if hit:
                current = hit[0]
            elif current:
                sections[current].append(line)
    sections[name] = list(lines)
    with open(path, "w") as f:
        for k, h in HEADS.items():
            if sections[k]:
                f.write("\n".join([h] + sections[k]) + "\n")


def main():
    if "--device-search" in sys.argv:
        return search_main()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    if "--resources" in sys.argv:
        write_section(out, "resources", resources("gpt_batch", "bat_factor"))
    if "--gpu" in sys.argv:
        lines, ratio = gpu()
        write_section(out, "measurements", lines)
        print("\n".join(lines))
        sys.exit(0 if ratio <= 8 else 1)


if __name__ == "__main__":
    main()
