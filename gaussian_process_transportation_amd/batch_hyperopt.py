"""Hyper-parameter search for a batch of small models (GaussianProcessBatch with optimizer='fmin_l_bfgs_b').

Every model gets what scikit-learn's protocol gives it alone (sklearn/gaussian_process/_gpr.py:296-338, as hyperopt.py):
L-BFGS-B on the negative log-marginal likelihood in theta = log(hyper-parameters), first from the kernel's own theta, then
from `n_restarts_optimizer` points drawn log-uniformly inside the bounds with the GLOBAL numpy RNG, the best optimum kept.
The driver stays scipy's L-BFGS-B; what changes is who evaluates the objective.  Every (model, start point) pair is one run
on a thread of its own, and its objective callback hands (model, theta) to a coalescer and blocks.  Once every live run is
waiting, the coalescer evaluates all pending requests with ONE gpt_batch_lml_objective call — one workgroup per request —
and hands the results back.  A model's objective does not depend on the batch around it (bit for bit), so every run sees the
values it would see alone and ends at the same optimum whatever the number of runs driven at once.

optimizer='device_bfgs' (opt-in) keeps the protocol — the same start points from the same RNG draws, the best run per model —
and hands all runs to gpt_batch_optimize, which carries each through a projected BFGS iteration on the device."""
from __future__ import annotations

import os
import threading
import warnings

import numpy as np
import scipy.optimize

from . import _lib
from .hyperopt import _free_mask, _make_unpack, _unpack


def _live_run_cap():
    """Runs driven at once (GPT_BATCH_OPT_RUNS, default 64): their threads sleep while the GPU works, so the cap bounds
    threads and the size of one batched call, not CPU load."""
    return max(1, int(os.environ.get("GPT_BATCH_OPT_RUNS", "64")))


THREAD_PREFIX = "gpt-batch-opt-"               # the run threads' names


def _stall_seconds():
    """How long the server waits for the live runs without any of them asking or ending before it gives up
    (GPT_BATCH_OPT_STALL_S, default 120): between two requests a run only does L-BFGS-B's own arithmetic, milliseconds."""
    return float(os.environ.get("GPT_BATCH_OPT_STALL_S", "120"))


DEVICE_SEARCH = "device_bfgs"                  # the opt-in search that runs on the device (gpt_batch_optimize)


def check_optimizer(optimizer):
    """Refuses what cannot drive a batch (None, meaning no search, is the caller's business)."""
    if callable(optimizer):
        raise ValueError("a callable optimizer cannot drive a batch: its runs share threads and one batched objective, and "
                         "whether the callable is re-entrant is unknown.  Use optimizer='fmin_l_bfgs_b', or a loop of GaussianProcess")
    if optimizer is not None and optimizer not in ("fmin_l_bfgs_b", DEVICE_SEARCH):
        raise ValueError(f"Unknown optimizer {optimizer}.")            # sklearn/_gpr.py:668-669


def _device_search(kernel, runs, free, n_ls, X_all, Y_all, n_begin, alpha, kernel_type, device, stats):
    """Every run carried through a projected BFGS iteration on the device, one workgroup per run (gpt_batch_optimize):
    [(theta (free components), f = -LML, warning or None)] in the order of `runs`, the shape of the scipy path's results."""
    fixed, bounds = _log_box(kernel, free)                         # (2 + n_ls, 2), log space; lo == hi: fixed
    theta0 = np.tile(fixed, (len(runs), 1))
    theta0[:, free] = np.array([t for _, t in runs])
    run_model = np.array([m for m, _ in runs], dtype=np.int32)
    theta, lml, iters, evals, status, launches = _lib.batch_optimize_packed(X_all, Y_all, n_begin, n_ls, run_model, theta0, bounds, alpha,
                                                                            kernel_type, device)
    if stats is not None:
        stats.update(runs=len(runs), launches=int(launches), evaluations=int(np.sum(evals)))
    names = {_lib.GPT_OPT_MAX_ITER: "MAX_ITER", _lib.GPT_OPT_MAX_EVALS: "MAX_EVALS", _lib.GPT_OPT_LINESEARCH: "LINESEARCH"}
    out = []
    for r in range(len(runs)):
        msg = None
        if int(status[r]) in names:            # what the scipy path says of a non-zero status
            msg = (f"{DEVICE_SEARCH} failed to converge (status={int(status[r])}): {names[int(status[r])]} after {int(iters[r])} "
                   f"iterations and {int(evals[r])} evaluations")
        if status[r] == _lib.GPT_OPT_NOT_PD_START:
            out.append((np.array(runs[r][1]), np.inf, None))
        else:
            out.append((theta[r][free], -float(lml[r]), msg))
    return out


class _Coalescer:
    """Collects one objective request from every live run, serves them with one batched call, repeats.

    `live` counts the runs that have started and not ended.  The serving thread fires when `live` requests are pending: a
    run that has ended is no longer live, so nobody waits for it, and a run that ends while others wait makes the count
    match (its `run_ended` wakes the server).  Every call therefore serves exactly one request of every live run."""

    def __init__(self, evaluate):
        self.evaluate = evaluate              # [(run, theta)] -> [(value, gradient)]
        self.cond = threading.Condition()
        self.pending = []                     # [run, theta, result]
        self.live = 0
        self.calls = 0
        self.failed = False                   # the batched call raised: no further run is started

    def request(self, run, theta):            # a run's thread
        item = [run, np.array(theta, dtype=np.float64), None]
        with self.cond:
            self.pending.append(item)
            self.cond.notify_all()
            while item[2] is None:
                self.cond.wait()
        if isinstance(item[2], BaseException):
            raise item[2]
        return item[2]

    def run_ended(self):                      # a run's thread, last thing it does
        with self.cond:
            self.live -= 1
            self.cond.notify_all()

    def serve(self, start_next):
        """The calling thread: start_next() starts one more run (False when none is left or the cap is reached); returns
        when every run has ended."""
        with self.cond:
            while True:
                while start_next():
                    pass
                if self.live == 0:
                    return
                if len(self.pending) < self.live:
                    seen = (len(self.pending), self.live)
                    if not self.cond.wait(timeout=_stall_seconds()) and seen == (len(self.pending), self.live):
                        # a run neither asks nor ends: fail the waiting ones, so that their threads end, and tell the caller
                        err = RuntimeError(f"hyper-parameter search stalled: {self.live - len(self.pending)} of {self.live} live runs "
                                           "neither asked for the objective nor ended")
                        self.failed = True
                        for item in self.pending:
                            item[2] = err
                        self.pending = []
                        self.cond.notify_all()
                        raise err
                    continue
                batch, self.pending = self.pending, []
                try:
                    results = self.evaluate([(run, theta) for run, theta, _ in batch])
                    self.calls += 1
                except BaseException as e:     # every waiting run fails with it, ends, and serve() returns
                    results = [e] * len(batch)
                    self.failed = True
                for item, res in zip(batch, results):
                    item[2] = res
                self.cond.notify_all()


def optimize_hyperparameters_batch(kernel, Xs, Ys, alpha=1e-10, optimizer="fmin_l_bfgs_b", n_restarts_optimizer=0, kernel_type=0,
                                   device=0, stats=None):
    """One (c, ls, noise, lml) per model, each maximising its log-marginal likelihood as sklearn would from `kernel`.
    Xs, Ys: validated sequences of (n_b, D) / (n_b, O) float64 arrays.  stats (a dict, optional) receives the number of
    batched objective calls and of runs; with optimizer='device_bfgs' the numbers of runs, launches and objective evaluations."""
    check_optimizer(optimizer)
    B = len(Xs)
    p = kernel.get_params()
    n_ls = int(np.size(p["k1__k2__length_scale"]))
    if kernel.n_dims == 0:
        c, ls, noise = _unpack(kernel, kernel.theta)
        return [(c, ls.copy(), noise, None) for _ in range(B)]
    free = _free_mask(kernel, n_ls)
    unpack = _make_unpack(kernel, free, n_ls)
    bounds = kernel.bounds
    if n_restarts_optimizer > 0 and not np.isfinite(bounds).all():
        raise ValueError("Multiple optimizer restarts (n_restarts_optimizer>0) requires that all bounds are finite.")

    # start points in sklearn's order (_gpr.py:319-330), all drawn before any run starts: the RNG ends where a plain loop
    # of GaussianProcess.fit calls would leave it
    rng = np.random.mtrand._rand
    runs = []                                  # (model, theta_init)
    for m in range(B):
        runs.append((m, np.array(kernel.theta)))
        for _ in range(n_restarts_optimizer):
            runs.append((m, rng.uniform(bounds[:, 0], bounds[:, 1])))

    X_all, Y_all, n_begin = _lib.batch_pack(Xs, Ys, "optimize_hyperparameters_batch")
    rows = [np.arange(n_begin[m], n_begin[m + 1]) for m in range(B)]
    if optimizer == DEVICE_SEARCH:
        results = _device_search(kernel, runs, free, n_ls, X_all, Y_all, n_begin, alpha, kernel_type, device, stats)
        return _best_per_model(kernel, results, B, n_restarts_optimizer)
    sizes = np.diff(n_begin)

    def evaluate(requests):
        models = [runs[r][0] for r, _ in requests]
        idx = np.concatenate([rows[m] for m in models])
        nb = np.zeros(len(models) + 1, dtype=np.int64)
        np.cumsum(sizes[models], out=nb[1:])
        hyper = [unpack(theta) for _, theta in requests]
        lml, grad, status = _lib.batch_lml_objective_packed(
            X_all[idx], Y_all[idx], nb, np.array([h[1] for h in hyper]), np.array([h[0] for h in hyper]),
            np.array([h[2] for h in hyper]), alpha, kernel_type, device)
        out = []
        for k in range(len(models)):
            if status[k] != _lib.GPT_OK:       # _gpr.py:587-590: -inf LML, zero gradient
                out.append((np.inf, np.zeros(int(free.sum()))))
            else:
                out.append((-float(lml[k]), -grad[k][free]))
        return out

    co = _Coalescer(evaluate)
    results = [None] * len(runs)
    errors = []
    threads = []

    def drive(r):
        try:
            res = scipy.optimize.minimize(lambda theta: co.request(r, theta), runs[r][1], method="L-BFGS-B", jac=True, bounds=bounds)
            msg = None
            if res.status != 0:                # sklearn's _check_optimize_result("lbfgs", ...)
                msg = f"lbfgs failed to converge (status={res.status}): {res.message}"
            results[r] = (res.x, res.fun, msg)
        except BaseException as e:
            errors.append(e)
        finally:
            co.run_ended()

    cap = _live_run_cap()

    def start_next():
        if co.failed or len(threads) >= len(runs) or co.live >= cap:
            return False
        t = threading.Thread(target=drive, args=(len(threads),), daemon=True, name=THREAD_PREFIX + str(len(threads)))
        threads.append(t)
        co.live += 1
        t.start()
        return True

    co.serve(start_next)
    for t in threads:                          # every run has called run_ended, its last act: the joins are immediate
        t.join(timeout=10)
        if t.is_alive():
            raise RuntimeError(f"hyper-parameter search: run thread {t.name} did not end")
    if stats is not None:
        stats.update(calls=co.calls, runs=len(runs))
    if errors:
        raise errors[0]
    return _best_per_model(kernel, results, B, n_restarts_optimizer)


def _log_box(kernel, free):
    """(fixed, bounds): the kernel's full theta = log [c, l.., noise] and its box (2 + n_ls, 2) in log space, lo == hi where a
    component is fixed — what gpt_batch_optimize takes."""
    p = kernel.get_params()
    fixed = np.log(np.concatenate([[float(p["k1__k1__constant_value"])], np.atleast_1d(np.asarray(p["k1__k2__length_scale"], dtype=np.float64)),
                                   [float(p["k2__noise_level"])]]))
    if not np.isfinite(kernel.bounds).all():
        raise ValueError(f"optimizer='{DEVICE_SEARCH}' requires that all bounds are finite.")
    if not np.isfinite(fixed[~free]).all():
        raise ValueError(f"optimizer='{DEVICE_SEARCH}' searches in log space: a fixed hyper-parameter must be > 0")
    bounds = np.column_stack([fixed, fixed])
    bounds[free] = kernel.bounds
    return fixed, bounds


def optimize_hyperparameters_candidates(kernels, X, Y, alpha=1e-10, n_restarts_optimizer=0, kernel_type=0, device=0, stats=None):
    """The device search (gpt_batch_optimize_bounded) for a list of candidate kernels over ONE data set X (n, D), Y (n, O), n <= 128:
    what a host loop `for k in kernels: GaussianProcess(k, n_restarts_optimizer=...).fit(X, Y)` searches, in one call.  The model
    is shared (B = 1, every run's model is 0); a candidate's runs carry its own bounds.  The starts are drawn as that loop draws
    them, candidate by candidate: first the kernel's own theta, then n_restarts_optimizer draws rng.uniform(lo, hi) from the
    global numpy RNG, which therefore ends where the loop leaves it.  The kernels share their layout (n_ls, which components are
    fixed).  Returns one (c, ls, noise, lml, theta) per candidate, its best run (the first on ties), theta being the free
    components in the kernel's order.  stats (a dict, optional) receives runs, launches, evaluations."""
    if not kernels:
        raise ValueError("optimize_hyperparameters_candidates: no candidate kernel")
    n_ls = int(np.size(kernels[0].get_params()["k1__k2__length_scale"]))
    free = _free_mask(kernels[0], n_ls)
    if not free.any():
        raise ValueError("optimize_hyperparameters_candidates: every hyper-parameter is fixed, nothing to search")
    rng = np.random.mtrand._rand
    theta0, boxes = [], []
    for k in kernels:
        if int(np.size(k.get_params()["k1__k2__length_scale"])) != n_ls or not np.array_equal(_free_mask(k, n_ls), free):
            raise ValueError("optimize_hyperparameters_candidates: the candidate kernels must share n_ls and their fixed components")
        fixed, box = _log_box(k, free)
        starts = [np.array(k.theta)] + [rng.uniform(k.bounds[:, 0], k.bounds[:, 1]) for _ in range(n_restarts_optimizer)]
        for s in starts:
            full = fixed.copy()
            full[free] = s
            theta0.append(full)
            boxes.append(box)
    X_all, Y_all, n_begin = _lib.batch_pack([X], [Y], "optimize_hyperparameters_candidates")
    R, per = len(theta0), 1 + n_restarts_optimizer
    theta, lml, iters, evals, status, launches = _lib.batch_optimize_bounded_packed(
        X_all, Y_all, n_begin, n_ls, np.zeros(R, dtype=np.int32), np.array(theta0), np.array(boxes), alpha, kernel_type, device)
    if stats is not None:
        stats.update(runs=R, launches=int(launches), evaluations=int(np.sum(evals)))
    names = {_lib.GPT_OPT_MAX_ITER: "MAX_ITER", _lib.GPT_OPT_MAX_EVALS: "MAX_EVALS", _lib.GPT_OPT_LINESEARCH: "LINESEARCH"}
    out = []
    for k, kernel in enumerate(kernels):
        f = []
        for r in range(k * per, (k + 1) * per):
            if int(status[r]) in names:
                warnings.warn(f"{DEVICE_SEARCH} failed to converge (status={int(status[r])}): {names[int(status[r])]} after {int(iters[r])} "
                              f"iterations and {int(evals[r])} evaluations")
            f.append(np.inf if status[r] == _lib.GPT_OPT_NOT_PD_START else -float(lml[r]))
        best = k * per + int(np.argmin(f))                       # the tie rule of _best_per_model: the first
        t = theta[best][free]
        c, ls, noise = _unpack(kernel, t)
        out.append((c, ls, noise, -f[best - k * per], t))
    return out


def _best_per_model(kernel, results, B, n_restarts_optimizer):
    """results: (theta, f, warning or None) per run, a model's runs together.  Warns, then keeps each model's best run."""
    for _, _, msg in results:
        if msg:
            warnings.warn(msg)                 # on the caller's thread: the warnings module's state is global
    out = []
    per = 1 + n_restarts_optimizer
    for m in range(B):
        mine = results[m * per:(m + 1) * per]
        best = int(np.argmin([v for _, v, _ in mine]))
        c, ls, noise = _unpack(kernel, mine[best][0])
        out.append((c, ls, noise, -mine[best][1]))
    return out
