"""Whole paths of the transported policy, numpy in to numpy out: ONE call (TransportChain.rollout: gpt_rollout_policy, the loop
over the steps on the device) against the host loop it replaces — one TransportChain.transported_policy call per step with the x
of the step before as its guess and y += dt * vel in numpy (tests/rollout_restatement.rollout) — on the same fitted objects in
one session.  Shapes:
    2d      letter-S (N = 20) then the obstacle rings (N = 36), dynamics on the demonstration (N = 400), D = 2
            M = 1, T = 1000 (the reference's plot_traj_evolution) and the 10 x 10 grid of starts, T = 200
    large   N_map = 8192 twice, N_dyn = 512, D = 3 (seeded as tools/chain_timing.py seeds its models)   M = 1024, T = 64
Warm-up, then the median of --reps runs, the two paths interleaved.  Per line: the times, the launches of the device call, whether
the two paths agree bit for bit, and the one condition: the device call is not slower than the loop.  For the large shape also
the longest single launch: the wall time of a call whose T is one launch's worth of steps, copies included, for several values of
GPT_ROLLOUT_STEPS_PER_LAUNCH — the default (64) is chosen so that this stays well below 50 ms.
usage: python tools/rollout_timing.py [--shapes 2d large] [--reps 5] [--out FILE (appended)]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gaussian_process_transportation_amd import TransportChain, _lib  # noqa: E402
from tests import rollout_restatement as RO  # noqa: E402
from chain_timing import problem  # noqa: E402

STEPS_PER_LAUNCH = 64           # ROLLOUT_STEPS_PER_LAUNCH of csrc/gpt_rollout.h


def cases(shape):
    """(chain, dynamics, {label: (starts, guesses, T, dt)})."""
    trs, dyn, sets = problem(shape)
    chain = TransportChain(trs, verbose=False)
    if shape == "2d":
        g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
        twice = chain.transport(g["demo"])[0]
        lo, hi = twice.min(axis=0), twice.max(axis=0)
        xg, yg = np.meshgrid(np.linspace(lo[0], hi[0], 10), np.linspace(lo[1], hi[1], 10))
        return chain, dyn, {"M = 1, T = 1000": (np.ascontiguousarray(twice[:1]), np.ascontiguousarray(g["demo"][:1]), 1000, 1.0),
                            "M = 100 (10 x 10 grid), T = 200": (np.ascontiguousarray(np.column_stack([xg.ravel(), yg.ravel()])), None, 200, 1.0)}
    y = sets["M = 100000"]
    return chain, dyn, {"M = 1024, T = 64": (np.ascontiguousarray(y[:1024]), None, 64, 0.05)}


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
    names = ("path", "vel", "x", "steps_done", "status")
    for shape in a.shapes:
        chain, dyn, sets = cases(shape)
        trs = chain.methods
        for label, (y0, x0, T, dt) in sets.items():
            def device():
                t0 = time.perf_counter()
                path, info = chain.rollout(dyn, y0, T, dt=dt, x0=x0, return_info=True)
                return time.perf_counter() - t0, dict(info, path=path)

            def step(y, guess):
                vel, info = chain.transported_policy(dyn, y, x0=guess, return_info=True)
                return info["x"], vel, info["status"]

            def loop():
                t0 = time.perf_counter()
                out = RO.rollout(step, y0, T, dt=dt, x0=x0)
                return time.perf_counter() - t0, out
            say(f"== {shape}: N_map = {len(trs[0].delta_map.X)} + {len(trs[1].delta_map.X)}, N_dyn = {len(dyn.X)}, D = {chain.n_features}, {label}, "
                f"dt = {dt}; median of {a.reps} (min .. max), ms")
            times, res = {"device": [], "loop": []}, {}
            for fn in (device, loop):
                fn()                                                   # warm-up: code objects, staging, scratch
            for _ in range(a.reps):
                for name, fn in (("loop", loop), ("device", device)):
                    t, res[name] = fn()
                    times[name].append(t)
            med = {n: 1e3 * float(np.median(t)) for n, t in times.items()}
            same = all(np.array_equal(res["device"][k], res["loop"][k], equal_nan=k in ("path", "vel", "x")) for k in names)
            done = res["device"]["steps_done"]
            say(f"   host loop, one transported_policy call per step : {med['loop']:10.3f}  ({1e3 * min(times['loop']):.3f} .. {1e3 * max(times['loop']):.3f})")
            say(f"   one call (gpt_rollout_policy), {-(-T // STEPS_PER_LAUNCH)} launch(es)        : {med['device']:10.3f}  ({1e3 * min(times['device']):.3f} .. "
                f"{1e3 * max(times['device']):.3f})   -> {med['loop'] / med['device']:.1f} x; not slower than the loop: "
                f"{'yes' if med['device'] <= med['loop'] else 'NO'}; bit for bit the same: {'yes' if same else 'NO'}; "
                f"steps done: min {int(done.min())}, median {int(np.median(done))}, max {int(done.max())}")
        if shape != "large":
            continue
        y0 = sets["M = 1024, T = 64"][0]
        say(f"== {shape}: the longest launch, M = 1024: wall time of a call of ONE launch (T = the steps of a launch), copies included; median of {a.reps}, ms")
        for per in (64, 128, 256):
            os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"] = str(per)          # (read per call)
            chain.rollout(dyn, y0, per, dt=0.05)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                path, info = chain.rollout(dyn, y0, per, dt=0.05, return_info=True)
                ts.append(time.perf_counter() - t0)
            say(f"   {per:4d} steps in one launch : {1e3 * float(np.median(ts)):10.3f}  ({1e3 * min(ts):.3f} .. {1e3 * max(ts):.3f}); "
                f"trajectories complete: {int(np.sum(info['steps_done'] == per))} of {len(y0)}")
        del os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
