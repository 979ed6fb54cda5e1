"""The coalescing hyper-parameter search of a batch of small models (batch_hyperopt.py), on the CPU: the batched objective is
served by the oracle's log_marginal_likelihood in place of gpt_batch_lml_objective, as
test_hyperparameter_search_driver_sequential_and_concurrent stands in for `_lib.Handle`."""
import numpy as np
import pytest

from tests.conftest import assert_parity

SIZES = (7, 20, 33, 60, 20)


def _problems():
    rng = np.random.default_rng(11)
    Xs = [rng.uniform(0, 1, (n, 2)) for n in SIZES]
    Ys = [np.column_stack([np.sin(4 * X[:, 0]), np.cos(3 * X[:, 1]) * X[:, 0]]) + 0.02 * rng.standard_normal((len(X), 2)) for X in Xs]
    return Xs, Ys


def _kernels():
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C
    return (C(1.0) * RBF([0.5, 0.5]) + WhiteKernel(0.01), C(1.0) * RBF(0.5) + WhiteKernel(0.01, "fixed"))


class OracleObjective:
    """gpt_batch_lml_objective's Python face (_lib.batch_lml_objective_packed) computed by the CPU oracle; counts the calls.
    not_pd: (rows of the model, call number from which on it reports GPT_E_NOT_PD once)."""

    def __init__(self, not_pd_rows=None):
        self.calls = 0
        self.sizes = []
        self.not_pd_rows = not_pd_rows
        self.not_pd_done = False

    def __call__(self, X, Y, n_begin, length_scale, constant_value, noise_level, alpha, kernel_type=0, device=0):
        from oracle import gp_oracle as orc
        self.calls += 1
        B = len(n_begin) - 1
        self.sizes.append(B)
        ls = np.asarray(length_scale).reshape(B, -1)
        lml, grad, status = np.full(B, np.nan), np.full((B, 2 + ls.shape[1]), np.nan), np.zeros(B, dtype=np.int32)
        for b in range(B):
            Xb, Yb = X[n_begin[b]:n_begin[b + 1]], Y[n_begin[b]:n_begin[b + 1]]
            if self.not_pd_rows == len(Xb) and not self.not_pd_done and self.calls == 3:
                self.not_pd_done = True
                status[b] = -2
                continue
            theta = np.log(np.concatenate([[constant_value[b]], ls[b], [noise_level[b]]]))
            lml[b], grad[b] = orc.log_marginal_likelihood(theta, Xb, Yb, ls.shape[1], alpha=alpha)
        return lml, grad, status


def _run_threads_alive():
    import threading
    from gaussian_process_transportation_amd.batch_hyperopt import THREAD_PREFIX
    return [t.name for t in threading.enumerate() if t.name.startswith(THREAD_PREFIX) and t.is_alive()]


def _search(monkeypatch, kernel, cap, objective, seed=5):
    from gaussian_process_transportation_amd import _lib, batch_hyperopt
    monkeypatch.setattr(_lib, "batch_lml_objective_packed", objective)
    monkeypatch.setenv("GPT_BATCH_OPT_RUNS", str(cap))
    Xs, Ys = _problems()
    stats = {}
    np.random.seed(seed)
    out = batch_hyperopt.optimize_hyperparameters_batch(kernel, Xs, Ys, alpha=1e-10, n_restarts_optimizer=3, stats=stats)
    return out, np.random.uniform(), stats


@pytest.mark.parametrize("which", [0, 1], ids=["ard", "iso_fixed_noise"])
def test_batch_search_matches_sklearn_loop_for_any_cap(monkeypatch, which):
    from sklearn.gaussian_process import GaussianProcessRegressor
    kernel = _kernels()[which]
    Xs, Ys = _problems()
    res = {}
    for cap in (1, 3, 64):
        obj = OracleObjective()
        res[cap] = _search(monkeypatch, kernel, cap, obj) + (obj,)
    # (b) bit-identical optima and the same RNG state for every cap
    for cap in (3, 64):
        assert res[cap][1] == res[1][1], "RNG state differs"
        for a, b in zip(res[cap][0], res[1][0]):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    # (a) every model's optimum is what sklearn finds in a plain loop under the same seed
    np.random.seed(5)
    for m, (c, ls, noise, lml) in enumerate(res[64][0]):
        ref = GaussianProcessRegressor(kernel=kernel, alpha=1e-10, n_restarts_optimizer=3).fit(Xs[m], Ys[m])
        rp = ref.kernel_.get_params()
        assert lml == pytest.approx(ref.log_marginal_likelihood_value_, rel=1e-8), m
        assert c == pytest.approx(rp["k1__k1__constant_value"], rel=1e-4), m
        assert_parity(ls, np.atleast_1d(rp["k1__k2__length_scale"]), 1e-4, f"length-scales of model {m} vs sklearn")
        assert noise == pytest.approx(rp["k2__noise_level"], rel=1e-4), m
    assert np.random.uniform() == res[64][1], "the RNG does not end where the plain loop leaves it"
    # (c) with every run live at once a call serves one request of every live run: calls <= longest run + number of runs
    obj, stats = res[64][3], res[64][2]
    assert stats["runs"] == len(SIZES) * 4 and stats["calls"] == obj.calls
    assert obj.sizes[0] == stats["runs"]
    longest = _longest_single_run(kernel, Xs, Ys)
    print(f"batched calls {obj.calls}, longest single run {longest}, runs {stats['runs']}; cap 1: {res[1][3].calls} calls")
    assert obj.calls <= longest + stats["runs"]
    assert max(res[1][3].sizes) == 1 and max(res[3][3].sizes) <= 3
    assert _run_threads_alive() == []


def _longest_single_run(kernel, Xs, Ys):
    """The largest number of objective evaluations any one (model, start) run needs, each run driven alone."""
    import scipy.optimize
    from oracle import gp_oracle as orc
    from gaussian_process_transportation_amd.hyperopt import _free_mask, _make_unpack
    n_ls = int(np.size(kernel.get_params()["k1__k2__length_scale"]))
    free = _free_mask(kernel, n_ls)
    unpack = _make_unpack(kernel, free, n_ls)
    np.random.seed(5)
    longest = 0
    for X, Y in zip(Xs, Ys):
        starts = [kernel.theta] + [np.random.uniform(kernel.bounds[:, 0], kernel.bounds[:, 1]) for _ in range(3)]
        for th0 in starts:
            count = [0]

            def f(theta):
                count[0] += 1
                c, ls, noise = unpack(theta)
                v, g = orc.log_marginal_likelihood(np.log(np.concatenate([[c], ls, [noise]])), X, Y, n_ls, alpha=1e-10)
                return -v, -g[free]
            scipy.optimize.minimize(f, th0, method="L-BFGS-B", jac=True, bounds=kernel.bounds)
            longest = max(longest, count[0])
    return longest


def test_not_pd_model_leaves_the_others_untouched_and_no_thread_blocked(monkeypatch):
    """(d) One model reports NOT_PD at one theta (its run sees +inf and a zero gradient there, _gpr.py:587-590): the other
    models' optima are bit for bit what they are without the failure, and every thread ends."""
    kernel = _kernels()[0]
    clean, _, _ = _search(monkeypatch, kernel, 64, OracleObjective())
    obj = OracleObjective(not_pd_rows=33)
    hit, _, stats = _search(monkeypatch, kernel, 64, obj)
    assert obj.not_pd_done
    for m, n in enumerate(SIZES):
        if n == 33:
            continue
        a, b = hit[m], clean[m]
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3], m
    assert np.isfinite(hit[SIZES.index(33)][3])
    assert _run_threads_alive() == []


def test_failed_batched_call_ends_every_run(monkeypatch):
    """The batched call itself raising (a device error) reaches the caller and leaves no run waiting."""
    from gaussian_process_transportation_amd import _lib, batch_hyperopt

    def broken(*a, **k):
        raise _lib.GptError("gpt_batch_lml_objective failed (-1): stand-in")
    monkeypatch.setattr(_lib, "batch_lml_objective_packed", broken)
    monkeypatch.setenv("GPT_BATCH_OPT_RUNS", "3")
    Xs, Ys = _problems()
    stats = {}
    with pytest.raises(_lib.GptError):
        batch_hyperopt.optimize_hyperparameters_batch(_kernels()[0], Xs, Ys, n_restarts_optimizer=3, stats=stats)
    assert _run_threads_alive() == []


def test_a_run_that_never_asks_is_reported_not_waited_for_forever(monkeypatch):
    """A run blocked outside the objective (here: scipy's minimize replaced by a wait) makes the driver raise after the
    stall limit instead of hanging; the runs that were waiting are released and end."""
    import threading
    from gaussian_process_transportation_amd import _lib, batch_hyperopt
    release = threading.Event()
    real = batch_hyperopt.scipy.optimize.minimize
    first = []

    def minimize(f, x0, **kw):
        if not first:
            first.append(1)
            release.wait(30)                   # the stuck run; released at the end of the test
            raise RuntimeError("released")
        return real(f, x0, **kw)
    monkeypatch.setattr(batch_hyperopt.scipy.optimize, "minimize", minimize)
    monkeypatch.setattr(_lib, "batch_lml_objective_packed", OracleObjective())
    monkeypatch.setenv("GPT_BATCH_OPT_STALL_S", "0.5")
    Xs, Ys = _problems()
    try:
        with pytest.raises(RuntimeError, match="stalled: 1 of"):
            batch_hyperopt.optimize_hyperparameters_batch(_kernels()[0], Xs[:2], Ys[:2], n_restarts_optimizer=1)
    finally:
        release.set()
    for t in threading.enumerate():
        if t.name.startswith(batch_hyperopt.THREAD_PREFIX):
            t.join(timeout=5)
    assert _run_threads_alive() == []


def test_refusals_of_the_search():
    from sklearn.gaussian_process.kernels import RBF, WhiteKernel, ConstantKernel as C
    from gaussian_process_transportation_amd import batch_hyperopt
    Xs, Ys = _problems()
    with pytest.raises(ValueError, match="callable optimizer"):
        batch_hyperopt.optimize_hyperparameters_batch(_kernels()[0], Xs, Ys, optimizer=lambda f, x0, bounds: (x0, 0.0))
    with pytest.raises(ValueError, match="Unknown optimizer"):
        batch_hyperopt.optimize_hyperparameters_batch(_kernels()[0], Xs, Ys, optimizer="adam")
    unbounded = C(1.0, (1e-5, np.inf)) * RBF(0.5) + WhiteKernel(0.01)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match="requires that all bounds are finite"):
        batch_hyperopt.optimize_hyperparameters_batch(unbounded, Xs, Ys, n_restarts_optimizer=2)
    assert np.array_equal(np.random.get_state()[1], state)
    # nothing to optimise: the kernel's own values, no objective call
    fixed = C(1.0, "fixed") * RBF(0.5, "fixed") + WhiteKernel(0.01, "fixed")
    out = batch_hyperopt.optimize_hyperparameters_batch(fixed, Xs, Ys, n_restarts_optimizer=2)
    assert len(out) == len(Xs) and out[0][0] == 1.0 and out[0][3] is None
