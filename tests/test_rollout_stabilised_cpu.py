"""The variance-stabilised rollout restated in numpy (tests/rollout_stab_restatement.py) against the reference's own line and
against the mean rollout's restatement.  No GPU: the device call is held to these definitions by tests/test_rollout_stabilised.py."""
import numpy as np
from numpy.testing import assert_array_equal

from tests import inverse_map_restatement as INV
from tests import pullback_restatement as P
from tests import rollout_restatement as RO
from tests import rollout_stab_restatement as RS
from tests.conftest import load_golden

EPS = np.finfo(np.float64).eps


def _surface_dynamics():
    """The RBF dynamics of the 3-D demo on the oracle: demonstration -> its steps, as examples/dynamics_rollout_3d.py builds them
    (RBF: the reference applies the RBF formulas to any kernel)."""
    from oracle.gp_oracle import GaussianProcessOracle
    X = load_golden("surface_3d")["demo"]
    delta = np.zeros_like(X)
    delta[:-1] = X[1:] - X[:-1]
    return GaussianProcessOracle(np.sqrt(0.1), np.ones(3), 0.01).fit(X, delta), X


def test_one_step_is_the_reference_line():
    """gain 1: pos + (f - s ghat) equals pos + vel - std * grad / |grad| of plot_traj_evolution with the oracle's predict(return_std)
    and derivative_of_variance, to 8 ulps of the largest operand (the restatement takes the norm after scaling and s from var)."""
    dyn, X = _surface_dynamics()
    rng = np.random.default_rng(0)
    pos = np.concatenate([rng.uniform(X.min(axis=0), X.max(axis=0), (6, 3)), X[::150] + 0.01])
    off = np.sqrt(dyn.noise_level)
    worst = 0.0
    for p in pos:
        p = p.reshape(1, 3)
        vel, std = dyn.predict(p, return_std=True)
        std = float(np.asarray(std).reshape(-1)[0])
        grad = dyn.derivative_of_variance(p)[:, 0]
        want = p + vel.reshape(1, -1) - std * grad / np.linalg.norm(grad)
        var = np.array([(std + off) ** 2])
        fs = RS.stabilised(vel.reshape(1, 3), var, grad.reshape(1, 3), 1.0, off)
        got = p + fs
        tol = 8 * EPS * max(np.max(np.abs(p)), np.max(np.abs(vel)), abs(std) + off)
        worst = max(worst, float(np.max(np.abs(got - want)) / tol))
        assert np.all(np.abs(got - want) <= tol), (p, got, want)
    print(f"one step against the reference line: largest share of 8 ulps of the operands {worst:.3f}")
    # the restated variance terms are the oracle's
    vt = RS.variance_terms(dyn.X, dyn.constant_value, dyn.length_scale, dyn.noise_level, dyn.alpha, "rbf", pos)
    _, std = dyn.predict(pos, return_std=True)
    std = np.asarray(std).reshape(len(pos), -1)[:, 0]
    assert np.all(np.abs(np.sqrt(vt["var"]) - off - std) <= 1e-9 * np.sqrt(vt["scale_var"]))
    assert np.all(np.abs(vt["dvar"] - dyn.derivative_of_variance(pos).T) <= 1e-8 * np.max(vt["scale_dvar"]))


def _restated(dyn, gain, y0, T, dt):
    model = P.oracle_model(dyn)
    off = np.sqrt(dyn.noise_level)
    inner = lambda y, guess: (y.copy(), model.mean(y)[0].astype(np.float64), np.full(len(y), INV.CONVERGED, dtype=np.int32))

    def terms(x):
        vt = RS.variance_terms(dyn.X, dyn.constant_value, dyn.length_scale, dyn.noise_level, dyn.alpha, "rbf", x)
        return vt["var"], vt["dvar"]

    step = RS.stab_step(inner, terms, lambda x, v, y, guess: v, gain, off)
    return RS.rollout(step, y0, T, dt=dt), step, model


def test_gain_zero_is_the_mean_rollout():
    dyn, X = _surface_dynamics()
    y0 = np.ascontiguousarray(X[::100][:5] + 0.02)
    for dt in (1.0, -0.3):
        got, step, model = _restated(dyn, 0.0, y0, 4, dt)
        want = RO.rollout(RO.mean_step(model), y0, 4, dt=dt)
        for k in want:
            assert_array_equal(got[k], want[k], err_msg=k)
        assert len(step.seen) == 4 and np.all(step.seen[0][1] > 0) and np.all(np.any(step.seen[0][2] != 0, axis=1))
    # and a gain moves the path, down the variance: the first step ends where the variance is lower than after the mean step
    got, step, _ = _restated(dyn, 1.0, y0, 2, 1.0)
    mean_only, mstep, _ = _restated(dyn, 0.0, y0, 2, 1.0)
    assert np.all(step.seen[1][1] < mstep.seen[1][1])
    assert_array_equal(got["path"][:, 1], y0 + got["vel"][:, 0])


def test_unit_gradient():
    g = np.array([[0.0, 0.0, 0.0], [1e-200, 1e-200, 1e-200], [3.0, 0.0, -4.0], [0.0, -2.0, 0.0], [1e300, 1e300, 0.0],
                  [np.nan, 1.0, 0.0], [np.inf, 1.0, 0.0], [5e-324, 0.0, 0.0]])
    h = RS.unit_gradient(g)
    assert_array_equal(h[0], 0.0)                                   # the reference divides 0 by 0 here
    assert np.all(np.abs(h[1] - 1 / np.sqrt(3)) <= 2 * EPS) and abs(np.linalg.norm(h[1]) - 1) <= 4 * EPS     # (its squares underflow)
    assert np.all(np.abs(h[2] - np.array([0.6, 0.0, -0.8])) <= 2 * EPS)
    assert_array_equal(h[3], [0.0, -1.0, 0.0])
    assert np.all(np.abs(h[4] - np.array([np.sqrt(0.5), np.sqrt(0.5), 0.0])) <= 2 * EPS)        # (its squares overflow)
    assert np.all(np.isnan(h[5])) and np.all(np.isnan(h[6]))        # a g that is not finite ends the path at the next point
    assert_array_equal(h[7], [1.0, 0.0, 0.0])
    # D = 1 and D = 2
    assert_array_equal(RS.unit_gradient(np.array([[-3e-310], [0.0], [7.0]])), [[-1.0], [0.0], [1.0]])
    assert np.all(np.abs(RS.unit_gradient(np.array([[1e-180, -1e-180]])) - np.array([[1.0, -1.0]]) / np.sqrt(2)) <= 2 * EPS)
    # the stabilised mean: each operation rounded on its own, 0 where the gradient is
    f = np.array([[1.0, 2.0, 3.0]])
    assert_array_equal(RS.stabilised(f, np.array([0.25]), np.zeros((1, 3)), 2.0, 0.1), f)
    assert_array_equal(RS.stabilised(f, np.array([0.25]), np.array([[0.0, 5.0, 0.0]]), 2.0, 0.1), f - np.array([[0.0, 2.0 * (0.5 - 0.1), 0.0]]))
    assert np.all(np.isnan(RS.stabilised(f, np.array([0.25]), np.array([[np.nan, 5.0, 0.0]]), 2.0, 0.1)))


def test_restated_end_rule():
    """The end rule is the mean rollout's, around the stabilised step: a trajectory ends by its status, or where the stabilised
    velocity takes it out of the finite numbers; f, var and dvar are seen for the trajectories still alive only."""
    T = 5
    y0 = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [10.0, 10.0]])

    def inner(y, guess):
        # trajectory 0 (y < 0.5) never converges; 1 stalls once it has passed 3; 3 goes on
        status = np.where(y[:, 0] < 0.5, INV.MAX_PASSES, np.where((y[:, 0] >= 3.0) & (y[:, 0] < 3.5), INV.STALLED, INV.CONVERGED))
        return y - 10.0, np.ones_like(y), status.astype(np.int32)

    def terms(x):
        # trajectory 2 (x = y - 10 in [-6.5, -5.5) at its second step) meets a gradient that is not finite
        bad = (x[:, 0] >= -6.5) & (x[:, 0] < -5.5)
        dvar = np.where(bad[:, None], np.nan, np.array([[0.0, -1.0]]) * np.ones_like(x))
        return np.full(len(x), 0.25), dvar

    step = RS.stab_step(inner, terms, lambda x, v, y, guess: v, 2.0, 0.0)
    out = RS.rollout(step, y0, T, dt=2.0, x0=y0 + 7.0)
    # a step: vel = (1, 1) - 2 * 0.5 * (0, -1) = (1, 2).  0: ends at step 0.  1: 1 -> 3, stalled at step 1.  2: 2 -> 4, NaN at step 1.
    assert list(out["steps_done"]) == [0, 1, 1, T]
    assert list(out["status"]) == [INV.MAX_PASSES, INV.STALLED, INV.CONVERGED, INV.CONVERGED]
    assert_array_equal(out["vel"][3], np.tile([1.0, 2.0], (T, 1)))
    assert_array_equal(out["path"][3], np.array([10.0, 10.0]) + 2.0 * np.arange(T + 1)[:, None] * np.array([1.0, 2.0]))
    assert np.all(np.isnan(out["vel"][2, 1])) and np.all(np.isnan(out["path"][2, 2:])) and np.all(np.isfinite(out["x"][2, 1]))
    for m, done in enumerate(out["steps_done"]):
        assert np.all(np.isfinite(out["path"][m, :done + 1])) and np.all(np.isnan(out["path"][m, done + 1:]))
        assert np.all(np.isnan(out["x"][m, min(done + 1, T):]))
    assert [len(s[1]) for s in step.seen] == [4, 3, 1, 1, 1]
    none = RS.rollout(step, y0, 0)
    assert none["path"].shape == (4, 1, 2) and list(none["steps_done"]) == [0] * 4
