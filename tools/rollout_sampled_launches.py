"""The duration of every launch of k_rollout_sampled at the largest admitted shape, from the profiler's kernel trace: the numbers
behind ROLLOUT_SAMPLED_STEPS_PER_LAUNCH (csrc/gpt_rollout_sampled.h).  A step's cost grows with t, so the LAST launch of a path of
256 steps decides, and a difference of two wall times cannot resolve one launch; the kernel trace holds each launch on its own.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/rollout_sampled_launches.py run
    python tools/rollout_sampled_launches.py report DIR [--out FILE (appended)]

run     N_map = 8192 twice, N_dyn = 1024, D = 3, T = 256 (tools/rollout_timing.py's large shape).  First P = 1024 paths through the
        device entry (gpt_rollout_sampled_dev on torch tensors: one chunk, 64 workgroups per launch) with 1, 2, 4, 8 and 16 steps per
        launch, then once through the host entry with its defaults (the 1 GiB scratch budget cuts 1024 paths into chunks of 400,
        400 and 224: 25, 25 and 14 workgroups per launch).  Prints the plan as it goes; one call of each kind runs first, untimed.
report  reads the kernel trace (csv) of such a run and prints, per call, the first, the median, the last and the longest launch."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WINDOWS = (1, 2, 4, 8, 16)
T, P = 256, 1024


def run():
    import torch
    from gaussian_process_transportation_amd import _lib
    from rollout_timing import stab_cases
    chain, dyn, _, y0, _, _, dt = stab_cases("large")
    assert chain is not None and len(y0) == P and T == _lib.ROLLOUT_SAMPLED_MAX_T
    D = y0.shape[1]
    z = np.random.RandomState(1).standard_normal((P, T, D))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    keep, stages = [], []
    for m in chain.methods:
        a = m.affine_transform
        R, cs, cd = t(a.rotation_matrix), t(a.S_centroid), t(a.T_centroid)
        keep.append((R, cs, cd))
        stages.append((m.delta_map._handle, R.data_ptr(), cs.data_ptr(), cd.data_ptr(), float(a.scale), R.data_ptr()))
    h_last, hd = chain.methods[-1].delta_map._handle, dyn._handle
    yd, zd = t(y0), t(z)
    path = torch.empty((P, T + 1, D), dtype=torch.float64, device=dev)
    steps = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)

    def device_call(w):
        os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"] = str(w)              # (read per call)
        h_last.rollout_sampled_dev(stages, hd, yd.data_ptr(), zd.data_ptr(), P, T, dyn._noise, path.data_ptr(), steps.data_ptr(), status.data_ptr(), dt=dt)
        h_last.synchronize()
        return int((steps == T).sum().item())
    print(f"warm-up: device entry, 16 steps per launch: {device_call(16)} of {P} paths complete", flush=True)
    for w in WINDOWS:
        print(f"device entry, P = {P}, T = {T}, {w} steps per launch, {-(-T // w)} launches: {device_call(w)} of {P} paths complete", flush=True)
    del os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"]
    for label in ("warm-up: ", ""):
        _, info = chain.rollout_samples(dyn, y0, T, n_samples=1, dt=dt, normals=z[:, None], return_info=True)
        print(f"{label}host entry, defaults: {int(np.sum(info['steps_done'] == T))} of {P} paths complete", flush=True)


def report(directory, out):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no *kernel_trace.csv under {directory}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rd = csv.DictReader(fh)
            col = lambda *names: next(c for c in rd.fieldnames if c.lower() in names)
            name, start, end = col("kernel_name"), col("start_timestamp"), col("end_timestamp")
            grid, wg = col("grid_size_x", "grid_size"), col("workgroup_size_x", "workgroup_size")
            for r in rd:
                if "k_rollout_sampled" in r[name]:
                    rows.append((int(r[start]), int(r[end]), int(r[grid]) // int(r[wg])))
    rows.sort()
    ms = [(e - s) * 1e-6 for s, e, _ in rows]
    wgs = [g for _, _, g in rows]
    lines = [f"k_rollout_sampled: {len(rows)} launches in the kernel trace ({', '.join(os.path.basename(f) for f in files)}); durations in ms"]
    at = -(-T // 16)                                                       # the warm-up call of the device entry
    for w in WINDOWS:
        n = -(-T // w)
        d = ms[at:at + n]
        assert len(d) == n and set(wgs[at:at + n]) == {P // 16}, (w, len(d), set(wgs[at:at + n]))
        lines.append(f"   device entry, {P // 16} workgroups, {w:2d} steps per launch, {n:3d} launches: first {d[0]:8.3f}   median {float(np.median(d)):8.3f}   "
                     f"LAST {d[-1]:8.3f}   longest {max(d):8.3f}   sum {sum(d):9.1f}")
        at += n
    rest, rest_wg = ms[at:], wgs[at:]
    half = len(rest) // 2                                                  # the warm-up host call, then the one reported
    d, g = rest[half:], rest_wg[half:]
    lines.append(f"   host entry with its defaults (chunks of {sorted(set(g), reverse=True)} workgroups), {len(d)} launches: median {float(np.median(d)):8.3f}   "
                 f"longest {max(d):8.3f}   sum {sum(d):9.1f}")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "report"))
    ap.add_argument("directory", nargs="?")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "run":
        run()
    else:
        report(a.directory, a.out)
