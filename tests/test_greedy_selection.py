"""Greedy active-learning subset selection (gpt_select_greedy, ActiveLearningGaussianProcess) against the reference's
gaussian_process_al.py, through the fixtures of tests/golden/make_active_learning_fixtures.py.

The fixtures hold the reference class's own insertion sequences; the generator asserts for each that the two largest
variances differ by >= 1e-7 relative at every insertion, so the sequence is a property of the rule and not of rounding.
Pools without that guarantee are checked for optimality at every step instead (test_tie_robust_optimality)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT, assert_parity

CASES = ["pan_cloud", "uniform_2d", "matern52_3d", "uniform_5d"]
KTYPE = {0.0: 0, 0.5: 1, 1.5: 2, 2.5: 3}


def load_case(name):
    with np.load(os.path.join(GOLDEN, f"active_learning_{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def theta(g):
    return float(g["constant_value"]), np.asarray(g["length_scale"], np.float64), float(g["noise_level"]), float(g["alpha"])


def kstat(h2, nu):
    if nu == 0:
        return np.exp(-0.5 * h2)
    r = np.sqrt(h2)
    if nu == 0.5:
        return np.exp(-r)
    if nu == 1.5:
        return (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r)
    return (1 + np.sqrt(5) * r + 5.0 / 3.0 * h2) * np.exp(-np.sqrt(5) * r)


def pivoted_cholesky(X, ls, c, noise, alpha, n_total, initial=(), nu=0, forced=None):
    """numpy restatement of the reference's loop for fixed theta: pivoted Cholesky of the pool's kernel matrix with the
    diagonal pivot rule.  d is sklearn's y_var (white noise included).  `forced`: follow this sequence instead of the
    argmax.  Returns selected, d[p] at each step, residual d, and per step (argmax, max d, second d, alive[p])."""
    Xs = np.asarray(X, np.float64) / ls
    N = Xs.shape[0]
    P = np.zeros((N, n_total))
    d = np.full(N, c + noise)
    alive = np.ones(N, bool)
    selected, dsel, steps = [], [], []
    for j in range(n_total):
        dd = np.where(alive, d, -np.inf)
        amax = int(np.argmax(dd))                      # first occurrence: the lowest index among ties
        if forced is not None:
            p = int(forced[j])
        elif j < len(initial):
            p = int(initial[j])
        else:
            p = amax
        top = np.partition(dd, -2)[-2:] if N > 1 else np.array([-np.inf, dd[0]])
        steps.append((amax, float(top[1]), float(top[0]), bool(alive[p])))
        selected.append(p)
        dsel.append(d[p])
        col = (c * kstat(((Xs - Xs[p]) ** 2).sum(1), nu) - P[:, :j] @ P[p, :j]) / np.sqrt(d[p] + alpha)
        P[:, j] = col
        d = d - col ** 2
        alive[p] = False
    return np.array(selected), np.array(dsel), d, steps


def make_kernel(c, ls, noise, nu=0.0, bounds="fixed"):
    from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel, ConstantKernel as CK
    stat = RBF(ls, bounds) if nu == 0 else Matern(ls, bounds, nu=nu)
    return CK(c, bounds) * stat + WhiteKernel(noise, bounds)


def uniform_pool(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = 0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal((N, D))
    return X, Y


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_sequence(name):
    """The equivalence claim without a GPU: the pivoted-Cholesky restatement gives the reference class's insertion
    sequence index for index and its std^2 at each insertion to 1e-9 relative."""
    g = load_case(name)
    c, ls, noise, alpha = theta(g)
    n0, m = int(g["n_initial"]), int(g["n_samples_max"])
    assert float(g["min_gap"]) >= 1e-7                       # the generator's condition, recorded in the fixture
    sel, dsel, _, steps = pivoted_cholesky(g["X"], ls, c, noise, alpha, m, g["selected"][:n0], nu=float(g["nu"]))
    assert np.array_equal(sel, g["selected"])
    rel = np.max(np.abs(dsel[n0:] - g["selection_variance"]) / g["selection_variance"])
    print(f"{name}: std^2 relative error of the restatement {rel:.3e}")
    assert rel <= 1e-9
    assert all(s[1] < c + noise for s in steps[n0:])         # no saturated pool point


def test_signature_table_has_the_entry():
    from gaussian_process_transportation_amd import _lib
    res, args = _lib.SIGNATURES["gpt_select_greedy"]
    assert res is C.c_int and len(args) == 15
    with open(os.path.join(ROOT, "include", "gpt_hip.h")) as f:
        header = f.read()
    assert "int gpt_select_greedy(" in header and "gaussian_process_al.py:26-57" in header


def test_class_shape_and_refusals_without_a_device():
    import gaussian_process_transportation_amd as pkg
    from gaussian_process_transportation_amd import _lib, gaussian_process_al
    from gaussian_process_transportation_amd.gaussian_process import GaussianProcess as Exact
    assert gaussian_process_al.GaussianProcess is pkg.ActiveLearningGaussianProcess
    assert issubclass(pkg.ActiveLearningGaussianProcess, Exact)
    k = make_kernel(0.1, np.full(3, 0.2), 1e-4)
    gp = pkg.ActiveLearningGaussianProcess(k)
    assert (gp.alpha, gp.n_restarts_optimizer, gp.n_samples_max, gp.selection_theta) == (1e-10, 5, 20000, "initial")
    assert gp.selected_indices_ is None and gp.selection_variance_ is None
    with pytest.raises(ValueError, match="selection_theta"):
        pkg.ActiveLearningGaussianProcess(k, selection_theta="every_step")
    with pytest.raises(ValueError, match="n_samples_max"):
        pkg.ActiveLearningGaussianProcess(k, n_samples_max=0)
    X = np.random.default_rng(0).uniform(0, 1, (40, 3))
    with pytest.raises(ValueError, match="D = 1 .. 15"):
        _lib.select_greedy(np.zeros((40, 16)), np.ones(16), 0.1, 1e-4, 1e-10, 8)
    with pytest.raises(ValueError, match="cannot select 41 points from a pool of 40"):
        _lib.select_greedy(X, 0.2, 0.1, 1e-4, 1e-10, 41)
    with pytest.raises(ValueError, match="length_scale"):
        _lib.select_greedy(X, [0.1, 0.2], 0.1, 1e-4, 1e-10, 8)
    with pytest.raises(ValueError, match="n_total"):
        _lib.select_greedy(X, 0.2, 0.1, 1e-4, 1e-10, 4, initial=np.arange(5))


# ---------------------------------------------------------------------------------------------- GPU
def _select(g, **kw):
    from gaussian_process_transportation_amd import _lib
    c, ls, noise, alpha = theta(g)
    n0, m = int(g["n_initial"]), int(g["n_samples_max"])
    return _lib.select_greedy(g["X"], ls, c, noise, alpha, m, initial=g["selected"][:n0], kernel_type=KTYPE[float(g["nu"])], **kw)


def _fit_class(g, **kw):
    from gaussian_process_transportation_amd import ActiveLearningGaussianProcess
    c, ls, noise, alpha = theta(g)
    nu = float(g["nu"])
    gp = ActiveLearningGaussianProcess(make_kernel(c, ls, noise, nu), alpha=alpha, n_samples_max=int(g["n_samples_max"]),
                                       optimizer=None, verbose=False, **kw)
    np.random.seed(int(g["seed"]))
    return gp.fit(g["X"], g["Y"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_fixture_sequence_parity(name):
    """1. The reference's insertion sequence index for index, its std^2 to 1e-9 relative — through _lib and the class."""
    g = load_case(name)
    n0 = int(g["n_initial"])
    sel, selvar, _ = _select(g)
    rel = np.max(np.abs(selvar - g["selection_variance"]) / g["selection_variance"])
    print(f"{name}: selection variance relative error {rel:.3e}, first mismatch "
          f"{np.flatnonzero(sel != g['selected'])[:1]}")
    assert np.array_equal(sel, g["selected"])
    assert rel <= 1e-9
    gp = _fit_class(g)
    assert np.array_equal(gp.selected_indices_, g["selected"])           # the class draws the reference's initial subset
    assert np.array_equal(gp.selection_variance_, selvar)
    assert gp.selection_variance_.shape == (int(g["n_samples_max"]) - n0,)
    assert np.array_equal(gp.X, g["X"][g["selected"]]) and np.array_equal(gp.Y, g["Y"][g["selected"]])
    assert gp.n_samples == int(g["n_samples_max"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_fitted_model_on_the_subset(name):
    """2. predict / derivative of the model fitted on the selected subset against the reference's."""
    g = load_case(name)
    gp = _fit_class(g)
    mean, std = gp.predict(g["Xq"], return_std=True)
    assert_parity(mean, g["mean"], what=f"{name} mean")
    assert_parity(std, g["std"], what=f"{name} std")
    if float(g["nu"]) == 0:
        J, Jvar = gp.derivative(g["Xq"], return_var=True)
        assert_parity(J, g["J"], what=f"{name} J")
        assert_parity(Jvar, g["Jvar"], what=f"{name} Jvar")
        return
    # Matern: the fixture's J / Jvar are the reference's RBF formulas on a Matern k*, which the package does not reproduce
    # (it refuses, or gives the analytic derivatives on request: README limits).  The class keeps that rule and passes the
    # parent's option through; the analytic J is held to central differences of the class's own mean (step 1e-4 of
    # length-scales >= 0.5: truncation ~ h^2 / (6 l^2) < 1e-8 relative, rounding ~ 1e-13 / h = 1e-9).
    with pytest.raises(NotImplementedError):
        gp.derivative(g["Xq"])
    gpm = _fit_class(g, matern_derivatives=True)
    assert np.array_equal(gpm.selected_indices_, g["selected"])
    J, Jvar = gpm.derivative(g["Xq"], return_var=True)
    assert J.shape == g["J"].shape and Jvar.shape == g["Jvar"].shape and np.all(Jvar >= 0)
    h = 1e-4
    fd = np.stack([(gpm.predict(g["Xq"] + h * e) - gpm.predict(g["Xq"] - h * e)) / (2 * h) for e in np.eye(g["Xq"].shape[1])], axis=2)
    assert_parity(J, fd, what=f"{name} analytic J vs central differences")


def _check_optimal(X, ls, c, noise, alpha, m, initial, sel, resid, ties_need_lowest=False):
    """Replays the GPU's sequence on the CPU: every chosen point was alive and within 1e-9 relative of the largest
    variance; the residual variance agrees to 1e-9 of c.  No step is exempt."""
    assert np.array_equal(sel[:len(initial)], initial)
    assert len(set(sel.tolist())) == m
    _, dsel, d_cpu, steps = pivoted_cholesky(X, ls, c, noise, alpha, m, forced=sel)
    worst, n_ties = 0.0, 0
    for j in range(len(initial), m):
        amax, top, second, was_alive = steps[j]
        assert was_alive, f"step {j}: the chosen point had been selected before"
        worst = max(worst, (top - dsel[j]) / top)
        assert dsel[j] >= top * (1 - 1e-9), f"step {j}: chosen variance {dsel[j]!r} < largest {top!r}"
        if top == second:                                    # an exact tie on the CPU: numpy's argmax takes the lowest index
            n_ties += 1
            if ties_need_lowest:
                assert sel[j] == amax, f"step {j}: tie went to index {sel[j]}, numpy.argmax takes {amax}"
    err = np.max(np.abs(resid - d_cpu)) / c
    print(f"worst shortfall of a chosen variance {worst:.3e}, exact ties {n_ties}, residual variance error / c {err:.3e}")
    assert err <= 1e-9
    return n_ties


@pytest.mark.gpu
def test_tie_robust_optimality():
    """3. Pools without a gap guarantee: N = 50 000 x 3 with m = 1024, and the saturated 2000 x 3, l = 0.1 pool, where far
    from every selected point the variance stays at c + noise and many points tie bit for bit."""
    from gaussian_process_transportation_amd import _lib
    c, noise, alpha = 0.1, 1e-4, 1e-10
    for N, m, l, seed in [(50000, 1024, 0.2, 11), (2000, 120, 0.1, 0)]:
        X, _ = uniform_pool(N, 3, seed)
        initial = np.random.default_rng(seed + 1).choice(N, int(0.1 * m), replace=False)
        ls = np.full(3, l)
        sel, selvar, resid = _lib.select_greedy(X, ls, c, noise, alpha, m, initial=initial)
        _check_optimal(X, ls, c, noise, alpha, m, initial, sel, resid)


@pytest.mark.gpu
def test_rows_longer_than_the_staged_pivot_row():
    """Insertions beyond the 4096 pivot-row entries a workgroup stages in LDS read the pivot row's tail from global memory
    (the class's default n_samples_max = 20 000 spends most of its insertions there).  n_total = 4302: columns 4096 .. 4301,
    odd ones included — an odd j is where a lane's last 16-byte read of the pivot row also covers column j, which the
    row's owner writes in the same launch.  Same checks, same bounds as test_tie_robust_optimality; no step exempt."""
    from gaussian_process_transportation_amd import _lib
    c, noise, alpha = 0.1, 1e-4, 1e-10
    N, m = 6000, 4302
    X, _ = uniform_pool(N, 3, 61)
    initial = np.random.default_rng(62).choice(N, int(0.1 * m), replace=False)
    ls = np.full(3, 0.08)
    sel, selvar, resid = _lib.select_greedy(X, ls, c, noise, alpha, m, initial=initial)
    _check_optimal(X, ls, c, noise, alpha, m, initial, sel, resid)
    again = _lib.select_greedy(X, ls, c, noise, alpha, m, initial=initial)
    assert all(u.tobytes() == v.tobytes() for u, v in zip((sel, selvar, resid), again))


@pytest.mark.gpu
def test_exact_ties_take_the_lowest_index():
    """4. Duplicated pool rows and the saturated pool: wherever the two largest variances are bitwise equal on the CPU,
    the lowest pool index is taken, as numpy.argmax does."""
    from gaussian_process_transportation_amd import _lib
    c, noise, alpha = 0.1, 1e-4, 1e-10
    base, _ = uniform_pool(300, 3, 5)
    X = np.vstack([base, base[:100]])                         # rows 300 .. 399 repeat rows 0 .. 99
    initial = np.array([150, 200, 250, 299])
    ls = np.full(3, 0.3)
    sel, _, resid = _lib.select_greedy(X, ls, c, noise, alpha, 60, initial=initial)
    assert _check_optimal(X, ls, c, noise, alpha, 60, initial, sel, resid, ties_need_lowest=True) > 0
    X, _ = uniform_pool(2000, 3, 0)
    initial = np.random.default_rng(1).choice(2000, 12, replace=False)
    ls = np.full(3, 0.1)
    sel, _, resid = _lib.select_greedy(X, ls, c, noise, alpha, 120, initial=initial)
    assert _check_optimal(X, ls, c, noise, alpha, 120, initial, sel, resid, ties_need_lowest=True) > 0
    # no initial subset at all: every point ties at the prior variance and index 0 is the first pivot
    sel0, selvar0, _ = _lib.select_greedy(X, ls, c, noise, alpha, 5)
    assert sel0[0] == 0 and selvar0[0] == c + noise and selvar0.shape == (5,)


@pytest.mark.gpu
def test_prescribed_pivots_alone_give_the_posterior_variance():
    """5. n_total == n_initial: the residual variance is the predictive variance (white noise included) of the exact
    model fitted on the prescribed points, at every pool point — (std + sqrt(noise))^2 of the class's predict, which
    subtracts sqrt(noise) as the reference does.  Bound: 1e-9 of the prior variance c + noise (both sides are fp64 sums
    of 64 products of O(c) terms through a factor of condition number <= 64 c / noise < 1e5)."""
    from gaussian_process_transportation_amd import GaussianProcess, _lib
    c, noise, alpha = 0.1, 1e-4, 1e-10
    X, Y = uniform_pool(3000, 3, 21)
    subset = np.random.default_rng(22).choice(3000, 64, replace=False)
    ls = np.array([0.15, 0.2, 0.25])
    sel, selvar, resid = _lib.select_greedy(X, ls, c, noise, alpha, 64, initial=subset)
    assert np.array_equal(sel, subset) and selvar.shape == (0,)
    gp = GaussianProcess(make_kernel(c, ls, noise), alpha=alpha, optimizer=None, verbose=False).fit(X[subset], Y[subset])
    _, std = gp.predict(X, return_std=True)
    var = (std[:, 0] + np.sqrt(noise)) ** 2
    err = np.max(np.abs(resid - var)) / (c + noise)
    print(f"residual variance vs predict: max error / (c + noise) {err:.3e}")
    assert err <= 1e-9


@pytest.mark.gpu
def test_determinism_and_small_inputs_are_the_parent():
    """6. Two calls give identical bits; at or below n_samples_max the class is the parent class bit for bit."""
    from gaussian_process_transportation_amd import ActiveLearningGaussianProcess, GaussianProcess, _lib
    c, noise, alpha = 0.1, 1e-4, 1e-10
    X, Y = uniform_pool(20000, 3, 31)
    initial = np.random.default_rng(32).choice(20000, 30, replace=False)
    a = _lib.select_greedy(X, np.full(3, 0.2), c, noise, alpha, 300, initial=initial)
    b = _lib.select_greedy(X, np.full(3, 0.2), c, noise, alpha, 300, initial=initial)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    Xs, Ys = X[:400], Y[:400]
    Xq = np.random.default_rng(33).uniform(0, 1, (200, 3))
    k = make_kernel(c, np.full(3, 0.2), noise)
    al = ActiveLearningGaussianProcess(k, alpha=alpha, n_samples_max=400, optimizer=None, verbose=False).fit(Xs, Ys)
    ex = GaussianProcess(k, alpha=alpha, optimizer=None, verbose=False).fit(Xs, Ys)
    assert al.selected_indices_ is None and al.n_samples == 400
    for u, v in zip(al.predict(Xq, return_std=True) + al.derivative(Xq, return_var=True),
                    ex.predict(Xq, return_std=True) + ex.derivative(Xq, return_var=True)):
        assert u.tobytes() == v.tobytes()


@pytest.mark.gpu
def test_fit_initial_selects_with_the_fitted_theta():
    """7. selection_theta="fit_initial": the selection runs with the theta GaussianProcess.fit finds on the initial subset."""
    from gaussian_process_transportation_amd import ActiveLearningGaussianProcess, GaussianProcess, _lib
    X, Y = uniform_pool(3000, 2, 41)
    k = make_kernel(0.1, np.full(2, 0.3), 1e-3, bounds=(1e-5, 1e5))
    m = 300
    np.random.seed(5)
    al = ActiveLearningGaussianProcess(k, n_restarts_optimizer=1, n_samples_max=m, selection_theta="fit_initial",
                                       verbose=False).fit(X, Y)
    np.random.seed(5)
    initial = np.random.choice(range(3000), size=30, replace=False)
    gp0 = GaussianProcess(k, n_restarts_optimizer=1, verbose=False).fit(X[initial], Y[initial])
    c0, ls0, noise0 = gp0._c, gp0._ls, gp0._noise
    assert not np.allclose(ls0, 0.3)                          # the search moved theta
    sel, selvar, _ = _lib.select_greedy(X, ls0, c0, noise0, 1e-10, m, initial=initial)
    assert np.array_equal(al.selected_indices_, sel) and np.array_equal(al.selection_variance_, selvar)
    sel_given, _, _ = _lib.select_greedy(X, np.full(2, 0.3), 0.1, 1e-3, 1e-10, m, initial=initial)
    assert not np.array_equal(sel, sel_given)


def _raw(lib, X, ls, c, noise, alpha, initial, n_total, ktype=0):
    X = np.ascontiguousarray(X, np.float64)
    ls = np.ascontiguousarray(ls, np.float64)
    initial = np.ascontiguousarray(initial, np.int64)
    sel = np.zeros(max(n_total, 1), np.int64)
    sv = np.zeros(max(n_total, 1))
    ip = C.POINTER(C.c_int64)
    dp = C.POINTER(C.c_double)
    return lib.gpt_select_greedy(0, X.ctypes.data_as(dp), X.shape[0], X.shape[1], ls.ctypes.data_as(dp), c, noise, alpha, ktype,
                                 initial.ctypes.data_as(ip), initial.size, n_total, sel.ctypes.data_as(ip), sv.ctypes.data_as(dp), None)


@pytest.mark.gpu
def test_refusals():
    """8. Host-side checks and the kernel's non-PD flag; the device stays usable afterwards."""
    from gaussian_process_transportation_amd import ActiveLearningGaussianProcess, _lib
    lib = _lib.load()
    _lib.require_gpu()
    X, Y = uniform_pool(500, 3, 51)
    init = np.arange(4)
    # the C entry point itself
    assert _raw(lib, np.zeros((40, 16)), np.ones(16), 0.1, 1e-4, 1e-10, init, 8) == _lib.GPT_E_ARG
    assert "D must be 1 .. 15" in _lib.last_error()
    assert _raw(lib, X, np.ones(3), 0.1, 1e-4, 1e-10, init, 501) == _lib.GPT_E_ARG
    assert "from a pool of 500" in _lib.last_error()
    Xn = X.copy()
    Xn[17, 1] = np.nan
    assert _raw(lib, Xn, np.ones(3), 0.1, 1e-4, 1e-10, init, 8) == _lib.GPT_E_ARG
    assert "NaN or infinity" in _lib.last_error()
    assert _raw(lib, X, np.ones(3), 0.1, 1e-4, 1e-10, np.array([3, 5, 3]), 8) == _lib.GPT_E_ARG
    assert "listed twice" in _lib.last_error()
    assert _raw(lib, X, np.ones(3), 0.1, 1e-4, 1e-10, init, 8, ktype=7) == _lib.GPT_E_ARG
    # a pool factor beyond the memory share: 8 * 4e6 * 2e6 bytes = 64 TB
    big = np.random.default_rng(52).uniform(0, 1, (4_000_000, 1))
    with pytest.raises(ValueError, match="free memory"):
        _lib.select_greedy(big, 0.1, 0.1, 1e-4, 1e-10, 2_000_000, initial=init)
    # the share counts every buffer that grows with N, not the factor alone: with m = 2 the factor is 16 N bytes of
    # the 16 N + (8 D + 8 * 16 + 9) N the call allocates; refused from the sizes alone, before the pool is read or copied
    assert lib.gpt_select_greedy(0, big.ctypes.data_as(C.POINTER(C.c_double)), 2**31 - 300, 15, np.ones(15).ctypes.data_as(C.POINTER(C.c_double)),
                                 0.1, 1e-4, 1e-10, 0, None, 0, 2, np.zeros(2, np.int64).ctypes.data_as(C.POINTER(C.c_int64)),
                                 np.zeros(2).ctypes.data_as(C.POINTER(C.c_double)), None) == _lib.GPT_E_ARG
    assert "free memory" in _lib.last_error()
    # the Python layers
    with pytest.raises(ValueError, match="D = 1 .. 15"):
        ActiveLearningGaussianProcess(make_kernel(0.1, np.ones(16), 1e-4), n_samples_max=10, optimizer=None,
                                      verbose=False).fit(np.zeros((40, 16)), np.zeros((40, 1)))
    with pytest.raises(ValueError, match="NaN or infinity"):
        ActiveLearningGaussianProcess(make_kernel(0.1, np.ones(3), 1e-4), n_samples_max=50, optimizer=None,
                                      verbose=False).fit(Xn, Y)
    # not positive definite: two prescribed pivots at the same position, no noise and no jitter -> the second pivot's
    # residual variance is exactly 0 (c = 1: k(x, x) = 1 and 1 - 1 * 1 = 0 in any rounding)
    Xd = X.copy()
    Xd[1] = Xd[0]
    with pytest.raises(np.linalg.LinAlgError, match="non-positive pivot"):
        _lib.select_greedy(Xd, np.full(3, 0.2), 1.0, 0.0, 0.0, 10, initial=[0, 1, 2])
    # the device is usable afterwards, with no handle to repair
    c, noise, alpha, ls = 0.1, 1e-4, 1e-10, np.full(3, 0.3)
    sel, selvar, resid = _lib.select_greedy(X, ls, c, noise, alpha, 40, initial=init)
    _check_optimal(X, ls, c, noise, alpha, 40, init, sel, resid)
