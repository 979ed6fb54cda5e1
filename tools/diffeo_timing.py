"""Timing of the fold-free transport search (GaussianProcessTransportationDiffeo.optimize_diffeomorphism) on the letter-S demo:
search="device" (one gpt_batch_optimize_bounded call for all trials, one gpt_batch_fold_scan call to score them) against
search="host" (the trials as a loop over GaussianProcess fits scored in numpy with predict / derivative: existing code only).
numpy in to the fitted map at the chosen theta out (the whole optimize_diffeomorphism call, the final fit and its fold check
included in both), median of --reps, the two paths interleaved in one process, seed 0 before every call.

Cases: n_trials = 10 and 100; evaluation sets: the affine-moved trajectory (M = 400) and a 100 x 100 grid over its box +- 10.
Also: the launches of the device search, the wall time of a search cut to ONE launch (max_evals = evals_per_launch = 64, copies
included: an upper bound of the longest launch), the scan alone, and the README's rollout through the fold-free map.

    python tools/diffeo_timing.py [--reps 5] [--trials 10 100] [--out profiles/diffeo_search.txt]"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportationDiffeo, _lib  # noqa: E402
from gaussian_process_transportation_amd.batch_hyperopt import optimize_hyperparameters_candidates  # noqa: E402
from gaussian_process_transportation_amd.gaussian_process_transportation_diffeomorphic import trial_kernel  # noqa: E402


def transport(g):
    t = GaussianProcessTransportationDiffeo(verbose=False)
    t.source_distribution, t.target_distribution, t.training_traj = g["source"], g["target"], g["demo"]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    warnings.simplefilter("ignore")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    g = np.load(os.path.join(ROOT, "tests", "golden", "letterS_2d.npz"))
    t0 = transport(g)
    aff, X, Y = t0._prepare(False, True)
    traj = aff.predict(g["demo"])
    lo, hi = traj.min(0) - 10, traj.max(0) + 10
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 100), np.linspace(lo[1], hi[1], 100))
    sets = {"trajectory, M = 400": None, "100 x 100 grid, M = 10000": np.column_stack([gx.ravel(), gy.ravel()])}

    def run(search, n_trials, points):
        t = transport(g)
        np.random.seed(0)
        s = time.perf_counter()
        t.optimize_diffeomorphism(n_trials=n_trials, search=search, eval_points=points)
        return time.perf_counter() - s, t

    for n_trials in a.trials:
        for label, points in sets.items():
            say(f"== letter-S, n = {len(X)}, n_trials = {n_trials} (x 6 starts = {6 * n_trials} runs), criterion fold_free, {label}; median of {a.reps} "
                "(min .. max), ms")
            times, res = {"device": [], "host": []}, {}
            for search in ("device", "host"):
                run(search, n_trials, points)                          # warm-up: code objects, handles
            for _ in range(a.reps):
                for search in ("host", "device"):
                    dt, res[search] = run(search, n_trials, points)
                    times[search].append(dt)
            med = {k: 1e3 * float(np.median(v)) for k, v in times.items()}
            d, h = res["device"], res["host"]
            stats = d.diffeo_search_stats_
            say(f"   search=\"host\", {n_trials} GaussianProcess fits + numpy scoring      : {med['host']:10.2f}  ({1e3 * min(times['host']):.2f} .. {1e3 * max(times['host']):.2f})")
            say(f"   search=\"device\", one search call + one scan call             : {med['device']:10.2f}  ({1e3 * min(times['device']):.2f} .. "
                f"{1e3 * max(times['device']):.2f})   -> {med['host'] / med['device']:.1f} x; not slower than the host loop: "
                f"{'yes' if med['device'] <= med['host'] else 'NO'}")
            say(f"   device search: {stats['runs']} runs, {stats['launches']} launches, {stats['evaluations']} objective evaluations; the scan: 3 launches")
            say(f"   chosen max_lengthscale: device {d.max_lengthscale_:.4f}, host {h.max_lengthscale_:.4f}; fold-free on the evaluation set: device "
                f"{d.fold_free_}, host {h.fold_free_}; fold-free candidates: {int(np.sum(d.diffeo_trials_['n_fold'] == 0))} of {n_trials} "
                f"(host {int(np.sum(h.diffeo_trials_['n_fold'] == 0))}); n_fold equal in every trial: "
                f"{'yes' if np.array_equal(d.diffeo_trials_['n_fold'], h.diffeo_trials_['n_fold']) else 'NO'}; max |lml device - host| "
                f"{np.max(np.abs(d.diffeo_trials_['lml'] - h.diffeo_trials_['lml'])):.1e}")
        # the parts of the device path, n_trials candidates
        ms = np.geomspace(2, 20, n_trials)
        kernels = [trial_kernel(m, 2) for m in ms]
        np.random.seed(0)
        fits = optimize_hyperparameters_candidates(kernels, X, Y, n_restarts_optimizer=5)
        for label, points in sets.items():
            pts = traj if points is None else points
            t0._scan_device(X, Y, fits, pts)
            ts = []
            for _ in range(a.reps):
                s = time.perf_counter()
                t0._scan_device(X, Y, fits, pts)
                ts.append(time.perf_counter() - s)
            say(f"   the scan alone (gpt_batch_fold_scan, B = {n_trials}, surrogate, five numbers per candidate), {label}: "
                f"{1e3 * float(np.median(ts)):.3f}  ({1e3 * min(ts):.3f} .. {1e3 * max(ts):.3f})")
        Xp, Yp, nb = _lib.batch_pack([X], [Y])
        R = 6 * n_trials
        theta0 = np.tile(np.log([0.1, 2.0, 2.0, 1e-4]), (R, 1))
        boxes = np.tile(np.log(np.array([[1e-5, 1e5], [0.1, 20.0], [0.1, 20.0], [1e-5, 1e5]])), (R, 1, 1))
        ts = []
        for _ in range(a.reps + 1):
            s = time.perf_counter()
            out = _lib.batch_optimize_bounded_packed(Xp, Yp, nb, 2, np.zeros(R, dtype=np.int32), theta0, boxes, 1e-10, 0, max_evals=64, evals_per_launch=64)
            ts.append(time.perf_counter() - s)
        say(f"   a search call cut to ONE launch ({R} runs, at most 64 evaluations each, copies included; {out[5]} launch): "
            f"{1e3 * float(np.median(ts[1:])):.3f}  ({1e3 * min(ts[1:]):.3f} .. {1e3 * max(ts[1:]):.3f})")

    # the README's rollout (the demonstration's own dynamics, from the moved demonstration's start, 1000 steps of dt = 1)
    dyn = GaussianProcess(kernel=trial_kernel(20, 2).clone_with_theta(np.log([0.3, 1.5, 2.5, 0.01])), optimizer=None, verbose=False).fit(g["demo"], g["delta"])
    for name, kw in (("unconstrained fit (the fixture's theta)", dict(max_lengthscales=[20.0])), ("fold-free search, n_trials = 10", dict(n_trials=10))):
        t = transport(g)
        np.random.seed(0)
        t.optimize_diffeomorphism(**kw)
        moved = t.method.transport(g["demo"], return_std=False)[0]
        path, info = t.rollout_policy(dyn, moved[:1], 1000, dt=1.0, x0=g["demo"][:1], return_info=True)
        say(f"== rollout from the demonstration's start, T = 1000, {name}: max_lengthscale {t.max_lengthscale_:.2f}, fold-free on the trajectory "
            f"{t.fold_free_}, steps_done {int(info['steps_done'][0])}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
