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
--stabilised times the variance-stabilised rollout (variance_gain = 1: gpt_rollout_stabilised) instead, against the host loop of
the parent commit: per step predict(return_std=True) and derivative_of_variance of the dynamics (examples/dynamics_rollout_3d.py
--host) and, with maps, one transported_policy call before them and the push of the stabilised mean through its per-stage A in
numpy.  Shapes then: 3d (the demo dynamics, N = 460, M = 1, T = 1000), 2d (its 10 x 10 grid, T = 200) and large with N_dyn = 1024,
the largest the call admits, where the longest launch is measured for 16, 32 and 64 steps (the default is 32).
--sampled times the sampled rollout (gpt_rollout_sampled: rollout_samples) instead, against the host loop a user would write from
the calls that existed before it: per step and path predict(points so far, return_cov=True), np.linalg.cholesky and the draw from
the factor's last row (with maps: one transported_policy call per step for x, f and the per-stage A, and the push in numpy).  That
loop is serial in the paths, so on the larger shapes it is timed on the first --loop-paths paths and scaled to all of them, which
the line says.  Shapes: 3d (the demo dynamics, N = 460, M = 1, S = 32, T = 200), 2d (10 x 10 starts, S = 8, T = 100) and large
(N_map = 8192 twice, N_dyn = 1024, P = 1024, T = 64).  The per-launch times behind ROLLOUT_SAMPLED_STEPS_PER_LAUNCH come from the
profiler's kernel trace, not from wall times: tools/rollout_sampled_launches.py.
--pathwise times the rollout of whole drawn functions (gpt_rollout_pathwise: GaussianProcess.sample_functions, PosteriorFunctions.rollout,
TransportChain.rollout_functions; 2048 frequencies) against the numpy loop of the same functions (all paths of a step at once;
with maps one transported_policy call per step for x and the per-stage A, and the push in numpy) and, where that call admits the
shape, against rollout_samples with as many paths.  Shapes: 3d (N = 460, M = 1, S = 32, T = 200), 2d (10 x 10 starts, S = 8: 800
paths, T = 100, and T = 1000, which rollout_samples does not admit).  The time of sample_functions (one solve per function) is
on a line of its own.  --pathwise-launches: the calls behind ROLLOUT_PATHWISE_STEPS_PER_LAUNCH at the largest admitted shape (two
maps of 8192 points, N_dyn = 8192, J = 8192, D = 3, 1024 paths), one launch of 8, 16, 32, 64, 128 and 256 steps each, to be run under
`rocprofv3 --kernel-trace -f csv -d DIR --`; --pathwise-report DIR prints the launches of k_rollout_pathwise from that trace.
usage: python tools/rollout_timing.py [--stabilised | --sampled | --pathwise] [--shapes 2d large] [--reps 5] [--out FILE (appended)]"""
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


def stab_steps_per_launch():
    """As the call reads it: GPT_ROLLOUT_STEPS_PER_LAUNCH, else ROLLOUT_STAB_STEPS_PER_LAUNCH of csrc/gpt_rollout_stab.h."""
    v = os.environ.get("GPT_ROLLOUT_STEPS_PER_LAUNCH", "")
    return int(v) if v.isdigit() and int(v) >= 1 else 32


def stab_cases(shape):
    """(chain or None, dynamics, label, starts, guesses, T, dt) of the stabilised rollout."""
    from gaussian_process_transportation_amd import GaussianProcess
    from chain_timing import kernel
    if shape == "3d":
        X = np.load(os.path.join(ROOT, "tests", "golden", "surface_3d.npz"))["demo"]
        delta = np.zeros_like(X)
        delta[:-1] = X[1:] - X[:-1]
        dyn = GaussianProcess(kernel=kernel(np.sqrt(0.1), [1.0, 1.0, 1.0], 0.01, 1.5), optimizer=None, verbose=False, matern_derivatives=True).fit(X, delta)
        start = np.random.default_rng(0).uniform(X.min(axis=0), X.max(axis=0)).reshape(1, 3)
        return None, dyn, "M = 1, T = 1000", start, None, 1000, 1.0
    if shape == "2d":
        chain, dyn, sets = cases("2d")
        y0, x0, T, dt = sets["M = 100 (10 x 10 grid), T = 200"]
        return chain, dyn, "M = 100 (10 x 10 grid), T = 200", y0, x0, T, dt
    trs, _, sets = problem("large")
    demo = np.random.default_rng(2).uniform(0.1, 0.9, (1024, 3))
    dyn = GaussianProcess(kernel=kernel(0.05, [0.3, 0.3, 0.3], 1e-4, 1.5), optimizer=None, verbose=False, matern_derivatives=True).fit(demo, 0.1 * np.cos(3 * demo))
    return TransportChain(trs, verbose=False), dyn, "M = 1024, T = 64", np.ascontiguousarray(sets["M = 100000"][:1024]), None, 64, 0.05


def stabilised_main(a, say):
    from tests import rollout_stab_restatement as RS
    for shape in a.shapes:
        chain, dyn, label, y0, x0, T, dt = stab_cases(shape)
        off, gain = np.sqrt(dyn._noise), 1.0
        R = [] if chain is None else [np.asarray(m.affine_transform.rotation_matrix) for m in chain.methods]

        def device():
            t0 = time.perf_counter()
            if chain is None:
                path, info = dyn.rollout(y0, T, dt=dt, return_info=True, variance_gain=gain)
            else:
                path, info = chain.rollout(dyn, y0, T, dt=dt, x0=x0, return_info=True, variance_gain=gain)
            return time.perf_counter() - t0, dict(info, path=path)

        def step(y, guess):
            if chain is None:
                x, f, status, A = y.copy(), None, np.zeros(len(y), dtype=np.int32), None
            else:
                _, info = chain.transported_policy(dyn, y, x0=guess, return_info=True)
                x, f, status, A = info["x"], info["f"], info["status"], info["stage_A"]
            mean, std = dyn.predict(x, return_std=True)
            grad = dyn.derivative_of_variance(x).T
            v = (mean if f is None else f) - gain * std.reshape(len(x), -1)[:, :1] * RS.unit_gradient(grad)
            for k in range(len(R)):                                    # B_k = A_k R_jac,k, stage 0 first
                v = np.einsum("mij,mj->mi", A[k], v @ R[k].T)
            return x, v, status

        def loop():
            t0 = time.perf_counter()
            out = RO.rollout(step, y0, T, dt=dt, x0=x0)
            return time.perf_counter() - t0, out
        n_map = "none" if chain is None else " + ".join(str(len(m.delta_map.X)) for m in chain.methods)
        say(f"== stabilised {shape}: N_map = {n_map}, N_dyn = {len(dyn.X)}, D = {y0.shape[1]}, {label}, dt = {dt}, gain = {gain}; "
            f"median of {a.reps} (min .. max), ms")
        times, res = {"device": [], "loop": []}, {}
        for fn in (device, loop):
            fn()
        for _ in range(a.reps):
            for name, fn in (("loop", loop), ("device", device)):
                t, res[name] = fn()
                times[name].append(t)
        med = {n: 1e3 * float(np.median(t)) for n, t in times.items()}
        done, done_l = res["device"]["steps_done"], res["loop"]["steps_done"]
        both = np.minimum(done, done_l)
        gap = max((float(np.max(np.abs(res["device"]["path"][m, :b + 1] - res["loop"]["path"][m, :b + 1]))) for m, b in enumerate(both)), default=0.0)
        say(f"   host loop, predict(return_std) + derivative_of_variance{'' if chain is None else ' + transported_policy'} per step : {med['loop']:10.3f}  "
            f"({1e3 * min(times['loop']):.3f} .. {1e3 * max(times['loop']):.3f})")
        say(f"   one call (gpt_rollout_stabilised), {-(-T // stab_steps_per_launch())} launch(es) : {med['device']:10.3f}  ({1e3 * min(times['device']):.3f} .. "
            f"{1e3 * max(times['device']):.3f})   -> {med['loop'] / med['device']:.1f} x; not slower than the loop: "
            f"{'yes' if med['device'] <= med['loop'] else 'NO'}; {1e3 * med['device'] / max(1, T):.1f} us per step of the call; largest gap between the two "
            f"paths over their common steps {gap:.3e}; steps done: min {int(done.min())}, median {int(np.median(done))}, max {int(done.max())} "
            f"(loop: min {int(done_l.min())}, max {int(done_l.max())})")
        if shape != "large":
            continue
        say(f"== stabilised {shape}: the longest launch, M = 1024, N_dyn = {len(dyn.X)}: wall time of a call of ONE launch (T = the steps of a launch), "
            f"copies included; median of {a.reps}, ms")
        for per in (16, 32, 64):
            os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"] = str(per)          # (read per call)
            chain.rollout(dyn, y0, per, dt=dt, variance_gain=gain)
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                path, info = chain.rollout(dyn, y0, per, dt=dt, return_info=True, variance_gain=gain)
                ts.append(time.perf_counter() - t0)
            say(f"   {per:4d} steps in one launch : {1e3 * float(np.median(ts)):10.3f}  ({1e3 * min(ts):.3f} .. {1e3 * max(ts):.3f}); "
                f"trajectories complete: {int(np.sum(info['steps_done'] == per))} of {len(y0)}")
        del os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"]


def sampled_main(a, say):
    for shape in a.shapes:
        chain, dyn, _, y0, x0, _, dt = stab_cases(shape)
        S, T = {"3d": (32, 200), "2d": (8, 100), "large": (1, 64)}[shape]
        M, D = y0.shape
        P = M * S
        z = np.random.RandomState(0).standard_normal((M, S, T, D))
        nug, noise = dyn._noise, dyn._noise
        R = [] if chain is None else [np.asarray(m.affine_transform.rotation_matrix) for m in chain.methods]
        n_loop = P if shape == "3d" else min(P, a.loop_paths)

        def device():
            t0 = time.perf_counter()
            if chain is None:
                path, info = dyn.rollout_samples(y0, T, n_samples=S, dt=dt, normals=z, return_info=True)
            else:
                path, info = chain.rollout_samples(dyn, y0, T, n_samples=S, dt=dt, normals=z, x0=x0, return_info=True)
            return time.perf_counter() - t0, dict(info, path=path)

        def loop():
            """The first n_loop paths (path index = m S + j), one at a time."""
            t0 = time.perf_counter()
            paths = np.full((n_loop, T + 1, D), np.nan)
            for p in range(n_loop):
                m, j = divmod(p, S)
                y, guess = y0[m:m + 1].copy(), None if x0 is None else x0[m:m + 1]
                paths[p, 0] = y[0]
                xs = np.zeros((0, D))
                for t in range(T):
                    if chain is None:
                        x, A = y, None
                    else:
                        _, info = chain.transported_policy(dyn, y, x0=guess, return_info=True)
                        if info["status"][0] != 0:
                            break
                        x, A = info["x"], info["stage_A"]
                    xs = np.concatenate([xs, x])
                    mean, cov = dyn.predict(np.ascontiguousarray(xs), return_cov=True)
                    cov = (cov[..., 0] if cov.ndim == 3 else cov) + (nug - noise) * np.eye(t + 1)
                    g = np.linalg.cholesky(cov)[t]
                    v = (mean[t] + g @ z[m, j, :t + 1])[None]
                    for k in range(len(R)):
                        v = np.einsum("mij,mj->mi", A[k], v @ R[k].T)
                    y = y + dt * v
                    if not np.all(np.isfinite(y)):
                        break
                    paths[p, t + 1], guess = y[0], x
            return time.perf_counter() - t0, paths
        n_map = "none" if chain is None else " + ".join(str(len(m.delta_map.X)) for m in chain.methods)
        say(f"== sampled {shape}: N_map = {n_map}, N_dyn = {len(dyn.X)}, D = {D}, M = {M} starts x S = {S} samples = {P} paths, T = {T}, dt = {dt}, "
            f"nugget = noise = {nug:g}; median of {a.reps} (min .. max), ms")
        times, res = {"device": [], "loop": []}, {}
        for fn in (device, loop):
            fn()
        for _ in range(a.reps):
            for name, fn in (("loop", loop), ("device", device)):
                t, res[name] = fn()
                times[name].append(t)
        med = {n: 1e3 * float(np.median(t)) for n, t in times.items()}
        scaled = med["loop"] * P / n_loop
        dev_paths = res["device"]["path"].reshape(P, T + 1, D)[:n_loop]
        both = np.isfinite(dev_paths) & np.isfinite(res["loop"])
        gap = float(np.max(np.abs(dev_paths - res["loop"])[both])) if np.any(both) else 0.0
        done = res["device"]["steps_done"]
        say(f"   host loop, predict(return_cov) + cholesky + draw per step and path{'' if chain is None else ' (+ transported_policy)'}, {n_loop} of {P} paths : "
            f"{med['loop']:10.3f}  ({1e3 * min(times['loop']):.3f} .. {1e3 * max(times['loop']):.3f})"
            + ("" if n_loop == P else f"   -> scaled to {P} paths: {scaled:.3f}"))
        say(f"   one call (gpt_rollout_sampled), all {P} paths : {med['device']:10.3f}  ({1e3 * min(times['device']):.3f} .. {1e3 * max(times['device']):.3f})"
            f"   -> {scaled / med['device']:.1f} x; slower than the loop: {'NO' if med['device'] <= scaled else 'YES'}; largest gap between the two over "
            f"their common steps {gap:.3e} (the dynamics amplifies rounding); steps done: min {int(done.min())}, max {int(done.max())}; "
            f"status counts {np.bincount(res['device']['status'].ravel(), minlength=5).tolist()}")


def pathwise_main(a, say):
    from tests import pathwise_restatement as PW
    kind_of = {0: "rbf", 2: "matern32", 3: "matern52"}
    for shape in a.shapes:
        chain, dyn, _, y0, x0, _, dt = stab_cases(shape)
        for S, T in {"3d": [(32, 200)], "2d": [(8, 100), (8, 1000)]}[shape]:
            M, D = y0.shape
            P = M * S
            t0 = time.perf_counter()
            fn = dyn.sample_functions(n_functions=S, n_frequencies=2048, random_state=0)
            t_draw = time.perf_counter() - t0
            R = [] if chain is None else [np.asarray(m.affine_transform.rotation_matrix) for m in chain.methods]
            kind = kind_of[dyn._ktype]

            def device():
                t0 = time.perf_counter()
                if chain is None:
                    path, info = fn.rollout(y0, T, dt=dt, return_info=True)
                else:
                    path, info = chain.rollout_functions(fn, y0, T, dt=dt, x0=x0, return_info=True)
                return time.perf_counter() - t0, dict(info, path=path)

            func = np.tile(np.arange(S), M)
            Vp, ap = fn.weights[func], fn.amplitudes[func]            # (P,N,D), (P,J,2,D)

            def step(y, guess, idx):
                if chain is None:
                    x, status, A = y.copy(), np.zeros(len(y), dtype=np.int32), None
                else:
                    _, info = chain.transported_policy(dyn, y, x0=guess, return_info=True)
                    x, status, A = info["x"], info["status"], info["stage_A"]
                theta = x @ fn.omega.T
                v = (np.einsum("pn,pnd->pd", PW.kernel_matrix(x, dyn.X, dyn._c, dyn._ls, kind), Vp[idx])
                     + np.einsum("pj,pjd->pd", np.cos(theta), ap[idx, :, 0]) + np.einsum("pj,pjd->pd", np.sin(theta), ap[idx, :, 1]))
                for k in range(len(R)):
                    v = np.einsum("mij,mj->mi", A[k], v @ R[k].T)
                return x, v, status

            def loop():
                """tests/rollout_restatement.rollout with the indices of the live paths handed to the step (a path has its own function)."""
                t0 = time.perf_counter()
                path = np.full((P, T + 1, D), np.nan)
                path[:, 0] = np.repeat(y0, S, axis=0)
                alive, guess = np.arange(P), None if x0 is None else np.repeat(x0, S, axis=0)
                for t in range(T):
                    if len(alive) == 0:
                        break
                    xt, vt, st = step(np.ascontiguousarray(path[alive, t]), guess, alive)
                    with np.errstate(over="ignore", invalid="ignore"):
                        nxt = path[alive, t] + dt * vt
                    go = (np.asarray(st) == 0) & np.all(np.isfinite(nxt), axis=1)
                    path[alive[go], t + 1] = nxt[go]
                    alive, guess = alive[go], np.ascontiguousarray(xt[go])
                return time.perf_counter() - t0, {"path": path}

            def exact():
                t0 = time.perf_counter()
                if chain is None:
                    dyn.rollout_samples(y0, T, n_samples=S, dt=dt)
                else:
                    chain.rollout_samples(dyn, y0, T, n_samples=S, dt=dt, x0=x0)
                return time.perf_counter() - t0, None
            calls = {"device": device, "loop": loop}
            if T <= _lib.ROLLOUT_SAMPLED_MAX_T and len(dyn.X) <= _lib.ROLLOUT_STAB_MAX_N:
                calls["exact"] = exact
            n_map = "none" if chain is None else " + ".join(str(len(m.delta_map.X)) for m in chain.methods)
            say(f"== pathwise {shape}: N_map = {n_map}, N_dyn = {len(dyn.X)}, D = {D}, M = {M} starts x S = {S} functions = {P} paths, T = {T}, dt = {dt}, "
                f"J = 2048; median of {a.reps} (min .. max), ms")
            say(f"   sample_functions, {S} functions (frequencies, amplitudes, one solve each) : {1e3 * t_draw:10.3f}  (once)")
            times, res = {n: [] for n in calls}, {}
            for f_ in calls.values():
                f_()
            for _ in range(a.reps):
                for name, f_ in calls.items():
                    t, res[name] = f_()
                    times[name].append(t)
            med = {n: 1e3 * float(np.median(t)) for n, t in times.items()}
            rng = lambda n: f"({1e3 * min(times[n]):.3f} .. {1e3 * max(times[n]):.3f})"
            dev_paths = res["device"]["path"].reshape(P, T + 1, D)
            both = np.isfinite(dev_paths) & np.isfinite(res["loop"]["path"])
            gap = float(np.max(np.abs(dev_paths - res["loop"]["path"])[both])) if np.any(both) else 0.0
            done = res["device"]["steps_done"]
            say(f"   numpy loop of the same functions{'' if chain is None else ' (+ transported_policy per step)'} : {med['loop']:10.3f}  {rng('loop')}")
            say(f"   one call (gpt_rollout_pathwise), {-(-T // 128)} launch(es) : {med['device']:10.3f}  {rng('device')}   -> {med['loop'] / med['device']:.1f} x; "
                f"slower than the loop: {'NO' if med['device'] <= med['loop'] else 'YES'}; {1e3 * med['device'] / max(1, T):.1f} us per step of the call; largest "
                f"gap between the two over their common steps {gap:.3e} (the dynamics amplifies rounding); steps done: min {int(done.min())}, max "
                f"{int(done.max())}")
            if "exact" in calls:
                say(f"   rollout_samples, as many paths (exact, each path a function of its own) : {med['exact']:10.3f}  {rng('exact')}   -> the pathwise call "
                    f"takes {med['device'] / med['exact']:.2f} x its time; slower than rollout_samples: {'NO' if med['device'] <= med['exact'] else 'YES'}")
            else:
                say(f"   rollout_samples does not admit this shape (n_steps <= {_lib.ROLLOUT_SAMPLED_MAX_T}, N_dyn <= {_lib.ROLLOUT_STAB_MAX_N})")


def pathwise_large():
    """(chain, dynamics of 8192 points, the drawn functions with 8192 frequencies, 1024 starts, dt)."""
    from gaussian_process_transportation_amd import GaussianProcess
    from chain_timing import kernel
    trs, _, sets = problem("large")
    demo = np.random.default_rng(2).uniform(0.1, 0.9, (8192, 3))
    dyn = GaussianProcess(kernel=kernel(0.05, [0.3, 0.3, 0.3], 1e-4, 1.5), optimizer=None, verbose=False).fit(demo, 0.1 * np.cos(3 * demo))
    fn = dyn.sample_functions(n_functions=8, n_frequencies=_lib.PATHWISE_MAX_FREQ, random_state=0)
    return TransportChain(trs, verbose=False), dyn, fn, np.ascontiguousarray(sets["M = 100000"][:128]), 0.05


def pathwise_launches(a, say):
    chain, dyn, fn, y0, dt = pathwise_large()
    say(f"== pathwise large: N_map = 8192 + 8192, N_dyn = {len(dyn.X)}, J = {fn.omega.shape[0]}, D = 3, {len(y0)} starts x {len(fn)} functions = "
        f"{len(y0) * len(fn)} paths; one call of ONE launch per window (T = the steps of a launch)")
    for per in (8, 8, 16, 32, 64, 128, 256):                         # (the first call is the warm-up)
        os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"] = str(per)          # (read per call)
        t0 = time.perf_counter()
        path, info = chain.rollout_functions(fn, y0, per, dt=dt, return_info=True)
        say(f"   {per:4d} steps in one launch : wall {1e3 * (time.perf_counter() - t0):10.3f} ms, copies included; paths complete: "
            f"{int(np.sum(info['steps_done'] == per))} of {info['steps_done'].size}")
    del os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"]


def pathwise_report(a, say):
    import csv
    import glob
    rows = []
    for f_ in glob.glob(os.path.join(a.pathwise_report, "**", "*kernel_trace.csv"), recursive=True):
        with open(f_) as fh:
            rows += [r for r in csv.DictReader(fh) if "k_rollout_pathwise" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    say(f"== launches of k_rollout_pathwise in the kernel trace, in order (the windows of --pathwise-launches: 8 (warm-up), 8, 16, 32, 64, 128, 256 steps), ms")
    for r in rows:
        say(f"   grid {r.get('Grid_Size', r.get('Grid_Size_X', '?'))} : {(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6:10.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=("2d", "large", "3d"), default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stabilised", action="store_true", help="the variance-stabilised rollout against its host loop")
    ap.add_argument("--sampled", action="store_true", help="the sampled rollout against its host loop")
    ap.add_argument("--pathwise", action="store_true", help="the rollout of whole drawn functions against its numpy loop and rollout_samples")
    ap.add_argument("--pathwise-launches", action="store_true", help="one launch of 8 .. 256 steps at the largest shape (run under the profiler)")
    ap.add_argument("--pathwise-report", default=None, metavar="DIR", help="the launches of k_rollout_pathwise in the kernel trace under DIR")
    ap.add_argument("--loop-paths", type=int, default=8, help="--sampled: paths the host loop is timed on where it is scaled")
    a = ap.parse_args()
    if a.shapes is None:
        a.shapes = ["3d", "2d"] if a.pathwise else ["3d", "2d", "large"] if a.stabilised or a.sampled else ["2d", "large"]
    if "3d" in a.shapes and not (a.stabilised or a.sampled or a.pathwise):
        ap.error("the 3d shape is the stabilised, the sampled and the pathwise rollout's")
    if a.pathwise and "large" in a.shapes:
        ap.error("--pathwise takes the shapes 3d and 2d; the large shape is --pathwise-launches'")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if a.pathwise_report:
        pathwise_report(a, say)
        a.shapes = []
    else:
        _lib.require_gpu()
    if a.pathwise:
        pathwise_main(a, say)
        a.shapes = []
    if a.pathwise_launches:
        pathwise_launches(a, say)
        a.shapes = []
    if a.stabilised:
        stabilised_main(a, say)
        a.shapes = []
    if a.sampled:
        sampled_main(a, say)
        a.shapes = []
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
