"""The numpy restatement of the sampled rollout (tests/rollout_sampled_restatement.py) anchored to scikit-learn and to the mean
rollout's restatement; no GPU.  The dynamics: the letter-S demonstration (tests/golden/letterS_2d.npz, `demo` -> `delta`, 400
points) with c = 0.3, l = (1.5, 2.5), the hyper-parameters of the rollout tests, and each of the four kernels."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import posterior_restatement as PR
from tests import rollout_restatement as RO
from tests import rollout_sampled_restatement as SR
from tests.conftest import load_golden
from tests.test_pullback_policy import sk_kernel

C, LS, NOISE, JITTER = 0.3, [1.5, 2.5], 0.01, 1e-10
NU = {"rbf": None, "matern12": 0.5, "matern32": 1.5, "matern52": 2.5}
EPS = SR.EPS


@pytest.fixture(scope="module")
def demo():
    g = load_golden("letterS_2d")
    return np.ascontiguousarray(g["demo"]), np.ascontiguousarray(g["delta"])


def _model(demo, kind, noise=NOISE, ty=np.float64):
    return SR.Model(demo[0], demo[1], C, LS, noise, JITTER, kind, ty)


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("nugget", [NOISE, 1e-6])
def test_factor_and_mean_against_sklearn(demo, kind, nugget):
    """At the restated path's own points (one path of 24 steps from the demonstration's start): G G^T is scikit-learn's
    predict(return_cov=True) with the diagonal moved from the noise level to the nugget, and f its mean.

    Tolerance, by the rule of tests/posterior_restatement.py: 16 max(e, 64 x 2^-52) x scale per element, scale = c + nugget for the
    covariance and sum_n |k*_n alpha_n| for the mean, e the largest deviation, in units of the scale, of EITHER fp64 computation
    (the restatement's covariance before it is factored, scikit-learn's) from the longdouble restatement at the same points: what
    fp64 costs this operation on these inputs (the Gram matrix of 400 points with noise 0.01 has a condition number near 1e4), as
    measured by the reference and not by the factor under test.  16 is the rule's margin for another order of the same sums."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    X, Y = demo
    m64 = _model(demo, kind)
    T = 24
    z = np.random.RandomState(5).standard_normal((1, T, 2))
    out = SR.rollout(m64, X[:1], z, T, nugget)
    assert out["steps_done"][0] == T and out["status"][0] == SR.CONVERGED
    xs = out["x"][0]
    G = out["chol"][0]
    assert np.all(np.triu(G, 1) == 0) and np.all(np.diag(G) > 0)
    sk = GaussianProcessRegressor(kernel=sk_kernel(C, LS, NOISE, NU[kind]), optimizer=None, alpha=JITTER).fit(X, Y)
    mean_sk, cov_sk = sk.predict(xs, return_cov=True)
    if cov_sk.ndim == 3:
        cov_sk = cov_sk[..., 0]
    cov_sk = cov_sk + (nugget - NOISE) * np.eye(T)
    ld = SR.path_terms(_model(demo, kind, ty=SR.LD), xs, nugget)
    f64 = SR.path_terms(m64, xs, nugget)
    scale = C + nugget
    e = max(float(np.max(np.abs(f64["cov"].astype(SR.LD) - ld["cov"]))), float(np.max(np.abs(cov_sk.astype(SR.LD) - ld["cov"])))) / scale
    tol = PR.MARGIN * max(e, PR.FLOOR_ULPS * EPS) * scale
    err = np.abs(G @ G.T - cov_sk)
    print(f"{kind} nugget {nugget:g}: fp64 against longdouble {e / EPS:.1f} ulps of c + nugget; |G G^T - sklearn| {float(err.max()) / scale / EPS:.1f} ulps, "
          f"bound {tol / scale / EPS:.1f}")
    assert np.all(err <= tol)
    # the factor of the longdouble restatement agrees too (the same bound), and the conditional variances are its squared diagonal
    assert np.all(np.abs(G @ G.T - (ld["chol"] @ ld["chol"].T).astype(np.float64)) <= tol)
    assert_array_equal(out["cvar"][0], f64["cvar"])
    assert np.all(np.abs(np.diag(G) ** 2 - out["cvar"][0]) <= 2 * EPS * out["cvar"][0])
    # the mean
    s_mean = np.abs(m64.kstar(xs))[:, :, None] * np.abs(m64.alpha)[None]
    s_mean = s_mean.sum(1)
    e_m = max(float(np.max(np.abs(f64["f"].astype(SR.LD) - ld["f"]) / s_mean)), float(np.max(np.abs(mean_sk.astype(SR.LD) - ld["f"]) / s_mean)))
    assert np.all(np.abs(out["f"][0] - mean_sk) <= PR.MARGIN * max(e_m, PR.FLOOR_ULPS * EPS) * s_mean)


@pytest.mark.parametrize("kind", PR.KINDS)
def test_zero_normals_are_the_mean_rollout(demo, kind):
    m = _model(demo, kind)
    y0 = np.ascontiguousarray(demo[0][::57][:6] + 0.02)
    T = 12
    for dt in (1.0, -0.5):
        got = SR.rollout(m, y0, np.zeros((len(y0), T, 2)), T, NOISE, dt=dt)
        want = RO.rollout(RO.mean_step(m), y0, T, dt=dt)
        for k in ("path", "vel", "x", "steps_done", "status"):
            assert np.all((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))), (kind, dt, k)    # (== : +0 and -0 agree)
        assert np.all(got["steps_done"] == T)


@pytest.mark.parametrize("kind", PR.KINDS)
def test_degenerate_rule(demo, kind):
    """nugget = 0 and a step too small to move the point: x_1 == x_0 bitwise, the second pivot is rounding noise, and every path
    ends at step 1 with DEGENERATE; what step 1 computed (x, f, pvar, cvar) is recorded, its vel and everything later is not."""
    m = _model(demo, kind)
    y0 = np.ascontiguousarray(demo[0][::80][:5])
    T = 4
    out = SR.rollout(m, y0, np.random.RandomState(1).standard_normal((5, T, 2)), T, 0.0, dt=1e-300)
    assert_array_equal(out["x"][:, 1], out["x"][:, 0])
    assert np.all(out["steps_done"] == 1) and np.all(out["status"] == SR.DEGENERATE)
    assert np.all(out["cvar"][:, 0] > SR.floor(C, 0.0)) and np.all(out["cvar"][:, 1] <= SR.floor(C, 0.0))
    assert np.all(np.isfinite(out["f"][:, 1])) and np.all(np.isfinite(out["pvar"][:, 1]))
    assert np.all(np.isnan(out["vel"][:, 1:])) and np.all(np.isnan(out["path"][:, 2:])) and np.all(np.isnan(out["chol"][:, 1:]))
    # with the nugget at the noise level the same points are no trouble
    ok = SR.rollout(m, y0, np.random.RandomState(1).standard_normal((5, T, 2)), T, NOISE, dt=1e-300)
    assert np.all(ok["steps_done"] == T) and np.all(ok["status"] == SR.CONVERGED)


@pytest.mark.parametrize("kind", ["matern52", "rbf", "matern12"])
@pytest.mark.parametrize("noise", [0.01, 1e-6])
def test_no_pivot_below_the_nugget(demo, kind, noise):
    """nugget = the noise level of the fit: mathematically cvar_t >= nugget, and over 200 steps of 8 paths no pivot falls below it;
    no path is degenerate."""
    m = _model(demo, kind, noise=noise)
    T, P = 200, 8
    out = SR.rollout(m, np.repeat(demo[0][:1], P, axis=0), np.random.RandomState(0).standard_normal((P, T, 2)), T, noise)
    assert np.all(out["status"] == SR.CONVERGED) and np.all(out["steps_done"] == T)
    low = float(np.min(out["cvar"]))
    print(f"{kind} nugget {noise:g}: smallest pivot {low:.6g}")
    assert low >= noise


def test_empirical_covariance_of_the_draws(demo):
    """2000 restated paths of 3 steps from one start (Matern 5/2, dt = 0.1): the empirical covariance of (fs_0, fs_1, fs_2), per
    output coordinate, against G G^T at the MEAN path's points.  To first order: a sampled path's points are those of the mean
    path moved by dt (fs - f) ~ 0.1 x 0.1 in units where the length scales are 1.5 and 2.5, which changes an entry of the covariance
    by under 1 % of it; the sampling error is larger.  For n Gaussian draws the sample covariance S_ij has the standard error
    se_ij = sqrt((C_ii C_jj + C_ij^2) / (n - 1)); the margin is 5 se_ij plus that 1 % of sqrt(C_ii C_jj).  The sample means are
    held to f of the mean path within 5 sqrt(C_ii / n) plus the same first-order term on the mean, 1 % of sqrt(C_ii)."""
    m = _model(demo, "matern52")
    n, T, dt = 2000, 3, 0.1
    y0 = np.repeat(demo[0][40:41], n, axis=0)
    out = SR.rollout(m, y0, np.random.RandomState(11).standard_normal((n, T, 2)), T, NOISE, dt=dt)
    mean_path = SR.rollout(m, y0[:1], np.zeros((1, T, 2)), T, NOISE, dt=dt)
    Cm = SR.path_terms(m, mean_path["x"][0], NOISE)["cov"]
    root = np.sqrt(np.outer(np.diag(Cm), np.diag(Cm)))
    se = np.sqrt((root ** 2 + Cm ** 2) / (n - 1))
    for d in range(2):
        fs = out["vel"][:, :, d]
        S = np.cov(fs.T)
        print(f"coordinate {d}: |S - C| / se = {np.round(np.abs(S - Cm) / se, 2).tolist()}")
        assert np.all(np.abs(S - Cm) <= 5 * se + 0.01 * root)
        assert np.all(np.abs(fs.mean(0) - mean_path["f"][0, :, d]) <= 5 * np.sqrt(np.diag(Cm) / n) + 0.01 * np.sqrt(np.diag(Cm)))
