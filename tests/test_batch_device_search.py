"""The device hyper-parameter search of a batch of small models (gpt_batch_optimize, optimizer='device_bfgs') on the GPU.

The yardstick is the unchanged gpt_batch_lml_objective: every run's result is re-evaluated with it.  Shapes are the smallest at
which the kernel can go wrong: n at both edges of both size classes (1, 2, 32 | 33, 128), D = 1, 3, 15 with one and with D
length-scales, O = 1 and 16, the four kernel types, a few dozen runs per call.

Tolerances.  RTOL_LML = 1e-9 is the cap tests/test_batch_precision.py holds the objective to against its own reference; between
the search's own LML and the yardstick at the returned theta only exp(theta) differs (device exp against numpy's, an ulp).  The
projected gradient of a PGTOL run may exceed pgtol by that re-evaluation's rounding: 2 pgtol.  TOL_BEST, the best-of-restarts
comparison with scikit-learn, is derived in tests/test_batch_device_search_cpu.py."""
import warnings

import numpy as np
import pytest

from tests import batch_search_restatement as rs
from tests.test_batch_device_search_cpu import tol_best

pytestmark = pytest.mark.gpu

RTOL_LML = 1e-9
PGTOL = 1e-5
SIZES = (1, 2, 32, 33, 128)
#          D, n_ls, O, kernel type, noise fixed
CONFIGS = [(1, 1, 1, 0, False), (3, 3, 16, 1, False), (3, 1, 1, 2, True), (15, 15, 1, 3, False), (15, 1, 16, 0, False)]
IDS = ["D1_rbf", "D3_ard_O16_matern12", "D3_iso_fixed_noise_matern32", "D15_ard_matern52", "D15_iso_O16_rbf"]


def _models(D, O, seed):
    rng = np.random.default_rng(seed)
    Xs = [rng.uniform(0, 1, (n, D)) for n in SIZES]
    W = rng.standard_normal((D, O))
    Ys = [np.sin(3 * X @ W) + 0.05 * rng.standard_normal((len(X), O)) for X in Xs]
    return Xs, Ys


def _problem(cfg, runs_per_model=6, seed=3):
    """Packed models, bounds, and R = 30 runs in model order: starts uniform in a box wider than the bounds (some get clipped)."""
    from gaussian_process_transportation_amd import _lib
    D, n_ls, O, ktype, fixed_noise = cfg
    Xs, Ys = _models(D, O, seed)
    X, Y, n_begin = _lib.batch_pack(Xs, Ys)
    P = 2 + n_ls
    bounds = np.log(np.array([[1e-2, 1e2]] + [[5e-2, 2e1]] * n_ls + [[1e-4, 1e-1]]))
    if fixed_noise:
        bounds[-1] = np.log(1e-2)
    rng = np.random.default_rng(seed + 1)
    run_model = np.repeat(np.arange(len(SIZES)), runs_per_model).astype(np.int32)
    theta0 = rng.uniform(bounds[:, 0] - 0.5, bounds[:, 1] + 0.5, (run_model.size, P))
    theta0[:, bounds[:, 0] == bounds[:, 1]] = bounds[bounds[:, 0] == bounds[:, 1], 0]
    return dict(X=X, Y=Y, n_begin=n_begin, n_ls=n_ls, ktype=ktype, bounds=bounds, run_model=run_model, theta0=theta0)


def _search(p, pick=None, **kw):
    from gaussian_process_transportation_amd import _lib
    pick = np.arange(p["run_model"].size) if pick is None else np.asarray(pick)
    return _lib.batch_optimize_packed(p["X"], p["Y"], p["n_begin"], p["n_ls"], p["run_model"][pick], p["theta0"][pick], p["bounds"], 1e-10,
                                      p["ktype"], **kw)


def _yardstick(p, run_model, theta, alpha=1e-10):
    """gpt_batch_lml_objective at (model, theta) pairs: (lml, gradient with respect to theta, status)."""
    from gaussian_process_transportation_amd import _lib
    sizes = np.diff(p["n_begin"])
    idx = np.concatenate([np.arange(p["n_begin"][m], p["n_begin"][m + 1]) for m in run_model])
    nb = np.zeros(len(run_model) + 1, dtype=np.int64)
    np.cumsum(sizes[run_model], out=nb[1:])
    v = np.exp(theta)
    return _lib.batch_lml_objective_packed(p["X"][idx], p["Y"][idx], nb, v[:, 1:-1], v[:, 0], v[:, -1], alpha, p["ktype"])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))


@pytest.fixture(scope="module", params=CONFIGS, ids=IDS)
def searched(request):
    p = _problem(request.param)
    return p, _search(p)


def test_every_run_against_the_objective(searched):
    p, (theta, lml, iters, evals, status, launches) = searched
    lo, hi = p["bounds"][:, 0], p["bounds"][:, 1]
    start = np.clip(p["theta0"], lo, hi)
    assert set(status.tolist()) <= {rs.PGTOL, rs.FTOL, rs.MAX_ITER, rs.MAX_EVALS, rs.LINESEARCH}, status
    # 1. inside the bounds; fixed components bitwise untouched
    assert (theta >= lo).all() and (theta <= hi).all()
    fixed = lo == hi
    assert np.array_equal(theta[:, fixed], p["theta0"][:, fixed])
    assert (evals >= 1).all() and (evals > iters).all() and launches >= 1
    # 2. the returned LML is the objective at the returned theta
    y_lml, y_grad, y_status = _yardstick(p, p["run_model"], theta)
    assert (y_status == 0).all()
    err = np.abs(lml - y_lml) / np.abs(y_lml)
    print(f"LML against the objective at the returned theta: largest relative difference {err.max():.2e}")
    assert (err <= RTOL_LML).all(), err
    # 3. never below the clipped start (to the rounding of the start's re-evaluation)
    s_lml, _, s_status = _yardstick(p, p["run_model"], start)
    assert (s_status == 0).all()
    assert (lml >= s_lml - RTOL_LML * np.abs(s_lml)).all(), (lml - s_lml).min()
    assert (lml > s_lml).sum() >= status.size // 2, "most runs must improve on their start"
    # 4. PGTOL means a small projected gradient of f = -LML
    g = -y_grad
    pg = np.abs(theta - np.clip(theta - g, lo, hi)).max(axis=1)
    done = status == rs.PGTOL
    print(f"statuses {np.bincount(status, minlength=6).tolist()}, evaluations {evals.min()} .. {evals.max()}, launches {launches}; "
          f"largest projected gradient of a PGTOL run {pg[done].max() if done.any() else 0:.2e}")
    assert (pg[done] <= 2 * PGTOL).all(), pg[done].max()


def test_a_run_does_not_depend_on_the_batch_or_the_slicing(searched):
    p, full = searched
    R = p["run_model"].size
    # 5. alone, and in a permuted batch
    for r in (0, 7, 17, R - 1):
        alone = _search(p, [r])
        assert _same(alone, [a[r:r + 1] for a in full[:5]]), r
    perm = np.random.default_rng(0).permutation(R)
    shuffled = _search(p, perm)
    assert _same(shuffled, [a[perm] for a in full[:5]])
    # 6. one evaluation per launch, seven, all of them
    for per_launch in (1, 7, 10 ** 6):
        sliced = _search(p, evals_per_launch=per_launch)
        assert _same(sliced, full), per_launch
        assert sliced[5] == rs.launches_of(full[3], np.diff(p["n_begin"])[p["run_model"]] > 32, per_launch)


def test_caps_end_a_run_with_their_status():
    p = _problem(CONFIGS[1])
    out = _search(p, max_evals=3)
    assert (out[3] <= 3).all() and set(out[4][out[3] == 3].tolist()) <= {rs.MAX_EVALS, rs.FTOL, rs.PGTOL}
    assert (out[4] == rs.MAX_EVALS).any()
    out = _search(p, max_iter=1)
    assert (out[2] <= 1).all() and (out[4] == rs.MAX_ITER).any()


def test_a_start_that_is_not_pd_ends_alone():
    """7a. Duplicated points with noise (1e-300: c + noise == c) and jitter at 0: the second pivot is c - c.  Every run of that
    model reports NOT_PD_START with lml = -inf and its clipped start; the other runs are bit for bit what they are without it."""
    from gaussian_process_transportation_amd import _lib
    rng = np.random.default_rng(2)
    good = [rng.uniform(0, 1, (n, 2)) for n in (5, 40)]
    dup = np.repeat(rng.uniform(0, 1, (3, 2)), 2, axis=0)
    Xs = [good[0], dup, good[1]]
    Ys = [np.sin(3 * X[:, :1]) for X in Xs]
    X, Y, n_begin = _lib.batch_pack(Xs, Ys)
    bounds = np.log(np.array([[1e-2, 1e2], [5e-2, 2e1], [1e-300, 1e-300]]))
    run_model = np.array([0, 1, 2, 1, 0, 2], dtype=np.int32)
    theta0 = rng.uniform(bounds[:, 0], bounds[:, 1], (6, 3))
    theta0[3, 1] = 99.0                                              # clipped to its bound
    out = _lib.batch_optimize_packed(X, Y, n_begin, 1, run_model, theta0, bounds, 0.0)
    bad = run_model == 1
    assert (out[4][bad] == rs.NOT_PD_START).all() and (out[1][bad] == -np.inf).all() and (out[3][bad] == 1).all()
    assert np.array_equal(out[0][bad], np.clip(theta0[bad], bounds[:, 0], bounds[:, 1]))
    assert (out[4][~bad] != rs.NOT_PD_START).all() and np.isfinite(out[1][~bad]).all()
    keep = np.flatnonzero(~bad)
    without = _lib.batch_optimize_packed(X, Y, n_begin, 1, run_model[keep], theta0[keep], bounds, 0.0)
    assert all(np.array_equal(a[keep], b) for a, b in zip(out[:5], without[:5]))


def test_a_first_step_into_a_matrix_that_is_not_pd_backtracks_and_improves():
    """7b. 32 equispaced points, a smooth target, no noise: from l = 0.06 the gradient asks for a longer length-scale, and the
    first full step (one unit in log l: l = 0.163) lands where the matrix is numerically singular.  The restatement says so on
    the CPU (its first trial is +inf, the halved one is accepted); on the device the yardstick refuses the same trial point,
    and the run comes back with a better LML than its start and more evaluations than a run without rejected trials has."""
    from gaussian_process_transportation_amd import _lib
    from oracle import gp_oracle as orc
    n = 32
    X = ((np.arange(n) + 0.5) / n)[:, None]
    Y = np.sin(2 * np.pi * X)
    theta0 = np.log([[1.0, 0.06, 1e-300]])
    bounds = np.log(np.array([[1.0, 1.0], [0.01, 10.0], [1e-300, 1e-300]]))
    n_begin = np.array([0, n], dtype=np.int64)

    def fun(z):
        v, g = orc.log_marginal_likelihood(z, X, Y, 1, alpha=0.0)
        return -v, -g
    trace = []
    rs.search(fun, theta0[0], bounds[:, 0], bounds[:, 1], trace=trace)
    assert trace[0][:2] == (0, 0) and trace[0][2] == np.inf and trace[1][:2] == (0, 1) and np.isfinite(trace[1][2])
    p = dict(X=X, Y=Y, n_begin=n_begin, ktype=0)
    s_lml, s_grad, s_status = _yardstick(p, [0], theta0, alpha=0.0)
    assert s_status[0] == 0
    g = -s_grad[0] * (bounds[:, 0] != bounds[:, 1])
    trial = np.clip(theta0[0] - min(1.0, 1.0 / np.linalg.norm(g)) * g, bounds[:, 0], bounds[:, 1])
    assert _yardstick(p, [0], trial[None], alpha=0.0)[2][0] == _lib.GPT_E_NOT_PD, "the first trial point must not be PD on the device"
    theta, lml, iters, evals, status, _ = _lib.batch_optimize_packed(X, Y, n_begin, 1, np.zeros(1, dtype=np.int32), theta0, bounds, 0.0)
    print(f"start {s_lml[0]:.3f} -> {lml[0]:.3f} at l = {np.exp(theta[0, 1]):.4f}: {iters[0]} iterations, {evals[0]} evaluations, status {status[0]}")
    assert status[0] != rs.NOT_PD_START and lml[0] > s_lml[0] + 1.0
    assert iters[0] >= 1 and evals[0] >= iters[0] + 2                # the start, one trial per iteration, and the rejected ones
    assert theta[0, 1] > theta0[0, 1]


@pytest.mark.parametrize("family", [0, 1, 2], ids=["ard", "iso_fixed_noise", "multi_frame"])
def test_best_of_restarts_against_sklearn(family):
    """8. For every model the best of (1 + 5) device runs reaches scikit-learn's best LML from the same seed, to TOL_BEST."""
    from gaussian_process_transportation_amd import batch_hyperopt
    name, kernel, Xs, Ys = rs.families()[family]
    ref = rs.sklearn_best(kernel, Xs, Ys)
    end_ref = np.random.uniform()
    np.random.seed(5)
    stats = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = batch_hyperopt.optimize_hyperparameters_batch(kernel, Xs, Ys, alpha=1e-10, optimizer="device_bfgs", n_restarts_optimizer=5,
                                                            stats=stats)
    assert np.random.uniform() == end_ref
    mine = np.array([o[3] for o in out])
    print(f"{name}: {stats}; shortfall against scikit-learn {(ref - mine).max():.2e} (largest), {(ref - mine).min():.2e} (smallest)")
    assert stats["runs"] == 6 * len(Xs)
    assert (ref - mine <= tol_best(ref)).all(), (ref - mine, tol_best(ref))


def test_transportation_batch_end_to_end():
    """9. Eight frame pairs through GaussianProcessTransportationBatch with the device search and with the scipy path: every
    model's LML within TOL_BEST, the moved trajectories within TRAJ_TOL (tests/test_batch_device_search_cpu.py)."""
    from gaussian_process_transportation_amd import GaussianProcessTransportationBatch
    from tests.test_batch_device_search_cpu import TRAJ_TOL, transport_pairs, transport_kernel
    pairs = transport_pairs()
    res = {}
    for optimizer in ("fmin_l_bfgs_b", "device_bfgs"):
        np.random.seed(0)
        tb = GaussianProcessTransportationBatch(kernel_transport=transport_kernel(), optimizer=optimizer)
        tb.source_distributions, tb.target_distributions, tb.training_trajs, tb.training_deltas = map(list, zip(*pairs))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tb.fit_transportations()
        tb.apply_transportations()
        res[optimizer] = (np.array(tb.regressor.log_marginal_likelihood_values_), tb.training_trajs, tb.regressor.optimizer_stats_)
    a, b = res["fmin_l_bfgs_b"], res["device_bfgs"]
    worst = max(float(np.max(np.abs(x - y))) for x, y in zip(a[1], b[1]))
    print(f"LML difference {np.abs(a[0] - b[0]).max():.2e}, trajectories {worst:.2e}; device search {b[2]}, scipy path {a[2]}")
    assert set(b[2]) == {"runs", "launches", "evaluations"}
    assert (np.abs(a[0] - b[0]) <= tol_best(a[0])).all(), a[0] - b[0]
    assert worst <= TRAJ_TOL
