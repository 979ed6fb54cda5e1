"""The fold-free transport search on the GPU: gpt_batch_optimize_bounded (a box per run) against the unchanged gpt_batch_optimize,
and GaussianProcessTransportationDiffeo end to end on the letter-S demo, device search against host search against scikit-learn.

TOL_BEST, the bound on a best-of-restarts LML against scikit-learn's, is the one the project already holds the device search to
(tests/test_batch_device_search_cpu.py: max(6.2e-9, 2.22e-9 max(1, |LML|))).  The letter-S facts the end-to-end test expects
(which candidates are fold-free, what either criterion picks) are established from scikit-learn alone in
tests/test_fold_scan_cpu.py, which also shows every det(I + J_psi) involved to be at least 6e-5 from zero."""
import warnings

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.test_batch_device_search_cpu import tol_best
from tests.test_fold_scan_cpu import CANDIDATES, letter_s_table

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------- a box per run
def _bounded_problem():
    """Two models (n = 20: small class, n = 40: large), R = 13 runs, three distinct boxes dealt round the runs; the starts are
    drawn from a box wider than any of them, so some are clipped."""
    from gaussian_process_transportation_amd import _lib
    rng = np.random.default_rng(21)
    Xs = [rng.uniform(0, 1, (n, 2)) for n in (20, 40)]
    Ys = [np.sin(3 * X @ rng.standard_normal((2, 2))) + 0.05 * rng.standard_normal((len(X), 2)) for X in Xs]
    X, Y, n_begin = _lib.batch_pack(Xs, Ys)
    boxes = np.log(np.array([[[1e-2, 1e2], [5e-2, 2e1], [5e-2, 2e1], [1e-4, 1e-1]],
                             [[1e-1, 1e1], [1e-1, 0.3], [1e-1, 0.5], [1e-3, 1e-3]],          # a low ceiling; the noise fixed
                             [[1e-3, 1e3], [0.2, 0.8], [0.2, 0.8], [1e-5, 1.0]]]))
    R = 13
    which = np.arange(R) % 3
    run_model = (np.arange(R) % 2).astype(np.int32)
    theta0 = rng.uniform(np.log(1e-3) - 0.5, np.log(1e2) + 0.5, (R, 4))
    fixed = boxes[which][:, :, 0] == boxes[which][:, :, 1]
    theta0[fixed] = boxes[which][:, :, 0][fixed]
    return dict(X=X, Y=Y, n_begin=n_begin, boxes=boxes, which=which, run_model=run_model, theta0=theta0)


def _bounded(p, pick, **kw):
    from gaussian_process_transportation_amd import _lib
    return _lib.batch_optimize_bounded_packed(p["X"], p["Y"], p["n_begin"], 2, p["run_model"][pick], p["theta0"][pick],
                                              p["boxes"][p["which"][pick]], 1e-10, 0, **kw)


def test_a_box_per_run_equals_the_shared_box_bit_for_bit():
    from gaussian_process_transportation_amd import _lib
    p = _bounded_problem()
    R = p["run_model"].size
    everything = np.arange(R)
    got = _bounded(p, everything)
    assert _lib.GPT_OPT_NOT_PD_START not in got[4].tolist() and np.all(np.isfinite(got[1])) and np.any(got[2] > 1)
    lo, hi = p["boxes"][p["which"]][:, :, 0], p["boxes"][p["which"]][:, :, 1]
    assert np.all(got[0] >= lo) and np.all(got[0] <= hi)                    # every result inside its own box
    assert np.any(p["theta0"] < lo) and np.any(p["theta0"] > hi)            # ... although some starts were outside it
    assert len({tuple(t) for t in np.round(got[0], 6)}) > 3                 # the boxes matter: the runs do not end in one place
    for k in range(3):                                                      # the unchanged entry point, that box shared
        pick = everything[p["which"] == k]
        want = _lib.batch_optimize_packed(p["X"], p["Y"], p["n_begin"], 2, p["run_model"][pick], p["theta0"][pick], p["boxes"][k], 1e-10, 0)
        for a, b in zip(got[:5], want[:5]):
            assert np.array_equal(a[pick], b), k
    perm = np.random.default_rng(1).permutation(R)
    for order in (perm, everything):                                        # run order[i] of the full call is run i of this one
        for epl in (1, 64):
            other = _bounded(p, order, evals_per_launch=epl)
            for a, b in zip(got[:5], other[:5]):
                assert np.array_equal(a[order], b), epl


def test_a_start_outside_its_own_box_is_clipped_to_it():
    """max_evals = 1: a run ends after the evaluation of its clipped start, which is what theta then holds."""
    p = _bounded_problem()
    everything = np.arange(p["run_model"].size)
    theta, lml, iters, evals, status, _ = _bounded(p, everything, max_evals=1)
    lo, hi = p["boxes"][p["which"]][:, :, 0], p["boxes"][p["which"]][:, :, 1]
    assert np.array_equal(theta, np.clip(p["theta0"], lo, hi)) and np.all(evals == 1)
    assert not np.array_equal(theta, p["theta0"])
    with pytest.raises(ValueError, match="lo <= hi"):
        from gaussian_process_transportation_amd import _lib
        crossed = p["boxes"][p["which"]].copy()
        crossed[12, 1] = crossed[12, 1, ::-1]
        _lib.batch_optimize_bounded_packed(p["X"], p["Y"], p["n_begin"], 2, p["run_model"], p["theta0"], crossed, 1e-10, 0)


# ------------------------------------------------------------------------------------------------------- letter-S, end to end
def _letter_s(**kw):
    from gaussian_process_transportation_amd import GaussianProcessTransportationDiffeo
    g = load_golden("letterS_2d")
    t = GaussianProcessTransportationDiffeo(verbose=False, **kw)
    t.source_distribution, t.target_distribution, t.training_traj = g["source"], g["target"], g["demo"]
    return g, t


@pytest.fixture(scope="module")
def searches():
    """optimize_diffeomorphism(n_trials=10) from seed 0, both searches and both criteria: {(search, criterion): (transport, RNG
    state after)}."""
    out = {}
    state = np.random.get_state()
    try:
        for search in ("device", "host"):
            for criterion in ("fold_free", "error"):
                g, t = _letter_s()
                np.random.seed(0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    t.optimize_diffeomorphism(n_trials=10, criterion=criterion, search=search)
                out[search, criterion] = (t, np.random.get_state())
    finally:
        np.random.set_state(state)
    return out


def test_letter_s_trials_device_against_host_against_sklearn(searches):
    rows = letter_s_table()                                 # scikit-learn alone, seed 0
    sk_lml = np.array([r["lml"] for r in rows])
    sk_folds = [r["traj"]["n_fold"] for r in rows]
    for criterion in ("fold_free", "error"):
        dev, host = searches["device", criterion][0].diffeo_trials_, searches["host", criterion][0].diffeo_trials_
        for name, t in (("device", dev), ("host", host)):
            assert np.allclose(t["max_lengthscale"], CANDIDATES) and t["status"].tolist() == [0] * 10
            for k in range(10):
                d = abs(t["lml"][k] - sk_lml[k])
                print(f"{criterion} {name} m={CANDIDATES[k]:.2f} lml {t['lml'][k]:.9f} (sklearn {sk_lml[k]:.9f}, off by {d:.1e} of {tol_best(sk_lml[k]):.1e}) "
                      f"folds {t['n_fold'][k]} min_det {t['min_det'][k]:+.4f} error {t['error'][k]:.3f}")
            bad = [(k, t["lml"][k], sk_lml[k]) for k in range(10) if not abs(t["lml"][k] - sk_lml[k]) <= tol_best(sk_lml[k])]
            assert not bad, (name, bad)
            assert t["n_fold"].tolist() == sk_folds, name
        assert all(abs(dev["lml"][k] - host["lml"][k]) <= tol_best(host["lml"][k]) for k in range(10))
        assert dev["n_fold"].tolist() == host["n_fold"].tolist()
    for search in ("device", "host"):
        assert round(searches[search, "fold_free"][0].max_lengthscale_, 2) == 4.31
        assert round(searches[search, "error"][0].max_lengthscale_, 2) == 2.00
        assert searches[search, "fold_free"][0].fold_free_ and not searches[search, "error"][0].fold_free_
    # the RNG ends where a host loop of the same fits leaves it, whichever search ran
    for criterion in ("fold_free", "error"):
        a, b = searches["device", criterion][1], searches["host", criterion][1]
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_the_fold_free_map_inverts_and_rolls_out(searches):
    from gaussian_process_transportation_amd import GaussianProcess, _lib
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    g = load_golden("letterS_2d")
    t = searches["device", "fold_free"][0]
    assert t.fold_free_ is True
    t.training_traj = g["demo"]
    t.apply_transportation()
    moved = t.training_traj
    assert np.array_equal(t.traj_rotated + t.delta_map_mean, moved) or np.allclose(t.traj_rotated + t.delta_map_mean, moved, rtol=0, atol=1e-12)
    x, info = t.inverse_transport(moved, x0=g["demo"], return_info=True)
    assert np.all(info["status"] == _lib.INV_CONVERGED) and np.all(info["det"] > 0)
    assert np.max(np.abs(x - g["demo"])) <= 1e-6
    t.training_traj = g["demo"]
    # the README's rollout: the demonstration's own dynamics, from the moved demonstration's start, 1000 steps of dt = 1
    dynamics = GaussianProcess(kernel=ConstantKernel(0.3) * RBF([1.5, 2.5]) + WhiteKernel(0.01), optimizer=None, verbose=False).fit(g["demo"], g["delta"])
    path, rinfo = t.rollout_policy(dynamics, moved[:1], 1000, dt=1.0, x0=g["demo"][:1], return_info=True)
    print("steps_done through the fold-free map:", int(rinfo["steps_done"][0]))
    assert int(rinfo["steps_done"][0]) > 112


def test_check_invertibility_reproduces_the_reference_number():
    """At the fixture's theta (the unconstrained fit): the reference's sum of |delta + delta_inv|, computed here with scikit-learn
    (332.37), to 1e-6 relative; 21 folds; training_traj untouched."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    g = load_golden("letterS_2d")
    kernel = ConstantKernel(float(g["constant_value"])) * RBF(g["length_scale"].tolist()) + WhiteKernel(float(g["noise_level"]))
    _, t = _letter_s(kernel_transport=kernel)
    t.fit_transportation(optimize=False)
    before = t.training_traj.copy()
    error = t.check_invertibility()
    X, Y = t.gp_delta_map.X, t.gp_delta_map.Y
    traj = t.affine_transform.predict(g["demo"])
    fwd = GaussianProcessRegressor(kernel=kernel, alpha=1e-10, optimizer=None).fit(X, Y)
    inv = GaussianProcessRegressor(kernel=kernel, alpha=1e-10, optimizer=None).fit(X + Y, -Y)
    delta = fwd.predict(traj)
    delta_inv = inv.predict(traj + delta)
    want = float(np.sum(np.linalg.norm(delta + delta_inv, axis=1)))
    print("check_invertibility", error, "scikit-learn", want)
    assert abs(error - want) <= 1e-6 * want and abs(want - 332.37) < 0.01
    assert t.n_fold_ == 21 and t.min_det_ < 0
    assert t.training_traj is g["demo"] or np.array_equal(t.training_traj, before)
    assert np.allclose(t.delta_map_mean, delta, rtol=0, atol=1e-6) and np.allclose(t.delta_map_inv_mean, delta_inv, rtol=0, atol=1e-6 * np.abs(delta_inv).max())
    assert np.allclose(t.traj_rotated_inv, traj + delta + delta_inv, rtol=0, atol=1e-4)


def test_the_device_search_refuses_what_it_cannot_hold():
    from gaussian_process_transportation_amd import GaussianProcessTransportationDiffeo
    rng = np.random.default_rng(0)
    t = GaussianProcessTransportationDiffeo(verbose=False)
    t.source_distribution = rng.uniform(0, 1, (129, 2))
    t.target_distribution = t.source_distribution + 0.05
    t.training_traj = rng.uniform(0, 1, (5, 2))
    with pytest.raises(ValueError, match=r'n <= 128.*search="host"'):
        t.optimize_diffeomorphism(n_trials=2)
    t.source_distribution = rng.uniform(0, 1, (12, 4))
    t.target_distribution = t.source_distribution + 0.05
    t.training_traj = rng.uniform(0, 1, (5, 4))
    with pytest.raises(ValueError, match=r'D <= 3.*search="host"'):
        t.optimize_diffeomorphism(n_trials=2)
    with pytest.raises(ValueError, match="criterion"):
        t.optimize_diffeomorphism(n_trials=2, criterion="best")
