"""What the fold-scan and fold-free-search tests stand on, checked without a GPU.

1. tests/fold_scan_restatement.py, the longdouble statement of gpt_batch_fold_scan: against a 40-digit mpmath evaluation from the
   definitions (1e-17, as tests/test_batch_precision.py holds its reference), against scikit-learn's predict for psi, against a
   central finite difference for J.
2. The input sets of tests/test_fold_scan.py meet the conditions their tolerances assume (tests/fold_scan_cases.py).
3. The facts about the letter-S demo that the search is built on, from scikit-learn alone: which length-scale ceilings give a
   fold-free map, what the reference's criterion picks, what the fold-free criterion picks.
4. The selection rules of optimize_diffeomorphism on hand-made tables."""
import functools
import warnings

import numpy as np
import pytest

from tests import fold_scan_cases as fc
from tests import fold_scan_restatement as fr
from tests.conftest import load_golden

LD = fr.LD


# ------------------------------------------------------------------------------------------------------- 1. the restatement
def _mp_scan(X, Y, c, ls, noise, jitter, Xq):
    """psi, J, det, z, err from the definitions at 40 digits: K^-1 by mpmath's inverse, the determinant by mpmath's det."""
    import mpmath as mp
    mp.mp.dps = 40
    f = mp.mpf
    n, D = X.shape
    lsv = [f(float(v)) for v in np.broadcast_to(ls, (D,))]
    c, noise, jitter = f(float(c)), f(float(noise)), f(float(jitter))

    def gram(P):
        K = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                K[i, j] = (c + noise) + jitter if i == j else c * mp.exp(-sum(((P[i][d] - P[j][d]) / lsv[d]) ** 2 for d in range(D)) / 2)
        return K

    def mean_jac(P, w, x):
        ks = [c * mp.exp(-sum(((P[k][d] - x[d]) / lsv[d]) ** 2 for d in range(D)) / 2) for k in range(n)]
        m = [sum(ks[k] * w[k, o] for k in range(n)) for o in range(D)]
        J = mp.matrix(D, D)
        for o in range(D):
            for d in range(D):
                J[o, d] = sum(ks[k] * (P[k][d] - x[d]) / lsv[d] ** 2 * w[k, o] for k in range(n))
        return m, J

    Xm = [[f(float(v)) for v in row] for row in X]
    Ym = mp.matrix(Y.tolist())
    Xs = [[f(float(v)) for v in row] for row in (X + Y)]      # the fp64 sum, as the entry point forms it
    alpha, beta = mp.inverse(gram(Xm)) * Ym, mp.inverse(gram(Xs)) * (-Ym)
    out = dict(psi=[], J=[], det=[], z=[], err=[])
    for row in Xq:
        x = [f(float(v)) for v in row]
        m, J = mean_jac(Xm, alpha, x)
        z = [x[d] + m[d] for d in range(D)]
        mi, _ = mean_jac(Xs, beta, z)
        out["psi"].append(m); out["J"].append([J[o, d] for o in range(D) for d in range(D)]); out["det"].append(mp.det(J + mp.eye(D)))
        out["z"].append(z); out["err"].append(mp.sqrt(sum((m[d] + mi[d]) ** 2 for d in range(D))))
    return out


def _mp_error(got, want):
    import mpmath as mp
    g = np.asarray(got, dtype=LD).reshape(-1)
    hi = g.astype(np.float64)
    lo = (g - hi.astype(LD)).astype(np.float64)
    w = [x for e in want for x in (e if isinstance(e, (list, tuple)) else [e])]
    assert len(w) == g.size
    den = max(abs(x) for x in w)
    return float(max(abs(mp.mpf(float(h)) + mp.mpf(float(l)) - x) for h, l, x in zip(hi, lo, w)) / den)


def test_restatement_against_mpmath_at_40_digits():
    """n = 6, D = 2, ARD: every per-query output of the restatement within 1e-17 of the 40-digit value (longdouble rounding at
    this size: eps = 1.1e-19, cond(K) <= c n / noise = 30, sums of 6 terms), and the reductions are numpy's over those arrays."""
    rng = np.random.default_rng(77)
    X, Y, ls, _, _ = fc.draw_model(rng, 6, 2, 2)
    c, noise = 0.1, 0.02
    Xq = np.concatenate([rng.uniform(-0.1, 1.1, (4, 2)), X[1:2]])
    got = fr.scan(X, Y, c, ls, noise, fc.JITTER, Xq)
    want = _mp_scan(X, Y, c, ls, noise, fc.JITTER, Xq)
    errors = {q: _mp_error(got[q], want[q]) for q in want}
    print({q: f"{e:.1e}" for q, e in errors.items()})
    assert max(errors.values()) <= 1e-17, errors
    assert got["min_det"] == got["det"].min() and got["argmin"] == int(np.argmin(got["det"])) and got["n_fold"] == int((got["det"] <= 0).sum())
    assert got["err_sum"] == got["err"].sum() and got["err_max"] == got["err"].max()


@pytest.mark.parametrize("D,n_ls", [(1, 1), (2, 2), (3, 1), (3, 3)])
def test_restatement_against_sklearn_and_a_finite_difference(D, n_ls):
    """psi and the surrogate's psi_inv(z) against scikit-learn's predict (1e-9: conventions, not precision); J against the central
    difference of the restatement's own psi in longdouble, h = 1e-6 (truncation h^2 |psi'''| / 6 ~ 1e-11, rounding eps / h = 1e-13)."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    rng = np.random.default_rng(5 + D)
    X, Y, ls, c, noise = fc.draw_model(rng, 30, D, n_ls)
    Xq = rng.uniform(-0.1, 1.1, (9, D))
    got = fr.scan(X, Y, c, ls, noise, fc.JITTER, Xq)
    kernel = ConstantKernel(c) * RBF(length_scale=ls.tolist() if n_ls > 1 else float(ls[0])) + WhiteKernel(noise)
    sk = GaussianProcessRegressor(kernel=kernel, alpha=fc.JITTER, optimizer=None).fit(X, Y)
    assert fc.relerr(sk.predict(Xq).reshape(9, D), got["psi"]) <= 1e-9
    z = got["z"].astype(np.float64)
    inv = GaussianProcessRegressor(kernel=kernel, alpha=fc.JITTER, optimizer=None).fit(X + Y, -Y)
    err = np.linalg.norm(sk.predict(Xq).reshape(9, D) + inv.predict(z).reshape(9, D), axis=1)
    assert fc.relerr(err, got["err"]) <= 1e-8
    h = LD(1e-6)
    alpha = fr._alpha(X, Y, c, ls, noise, fc.JITTER, LD)
    lsv = np.broadcast_to(ls, (D,)).astype(LD)
    for d in range(D):
        e = np.zeros(D, dtype=LD)
        e[d] = h
        up, _ = fr._mean_jac(X.astype(LD), alpha, LD(c), lsv, Xq.astype(LD) + e)
        dn, _ = fr._mean_jac(X.astype(LD), alpha, LD(c), lsv, Xq.astype(LD) - e)
        assert fc.relerr((up - dn) / (2 * h), got["J"][:, :, d]) <= 1e-9
    assert fc.relerr(np.linalg.det(got["J"].astype(np.float64) + np.eye(D)), got["det"]) <= 1e-12


# ------------------------------------------------------------------------------------------------------- 2. the input sets
@pytest.mark.parametrize("cid", fc.CASES)
def test_input_sets_meet_the_stated_conditions(cid):
    """Every set of tests/test_fold_scan.py: the fp64 evaluation within 1e-11 of the restatement in every quantity of every
    member, so that no tolerance reaches the 1e-9 cap; and a map that folds at some queries but not at all of them wherever a
    member has a tile of queries and more than two sources."""
    s = fc.case(cid)
    for b, e in enumerate(s["e_oracle"]):
        n, ref = len(s["Xs"][b]), s["ref"][b]
        assert max(e.values()) <= fc.ORACLE_BOUND, (cid, b, n, e)
        assert all(fc.tolerance(v, n) <= fc.CAP for v in e.values())
        M = len(fc.queries_of(s, b))
        if M >= fc.QT - 1 and n > 2:
            assert 0 < ref["n_fold"] < M, (cid, b, n, ref["n_fold"], M)


# ------------------------------------------------------------------------------------------------------- 3. the letter-S facts
CANDIDATES = np.geomspace(2, 20, 10)
DET_TOLERANCE = 1e-11                                      # what the device scan is held to on det at this size (test_fold_scan.py)


@functools.lru_cache(maxsize=None)
def letter_s_table():
    """The ten trials of optimize_diffeomorphism(n_trials=10) on the letter-S demo with scikit-learn alone, seed 0: per candidate
    the fitted hyper-parameters, the LML and the restatement's scan on the trajectory and on a 50 x 50 grid (box +- 10)."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    g = load_golden("letterS_2d")
    X, Y = g["gp_X"], g["gp_Y"]
    traj = float(g["scale"]) * ((g["demo"] - g["S_centroid"]) @ g["rotation"].T) + g["T_centroid"]
    lo, hi = traj.min(0) - 10, traj.max(0) + 10
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 50), np.linspace(lo[1], hi[1], 50))
    grid = np.column_stack([gx.ravel(), gy.ravel()])
    state = np.random.get_state()
    np.random.seed(0)
    rows = []
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                # sklearn: "the optimal value is close to the specified bound"
            for m in CANDIDATES:
                kernel = ConstantKernel(0.1) * RBF([2, 2], length_scale_bounds=[0.1, m]) + WhiteKernel(1e-4)
                gp = GaussianProcessRegressor(kernel=kernel, alpha=1e-10, n_restarts_optimizer=5).fit(X, Y)
                p = gp.kernel_.get_params()
                hyper = (p["k1__k1__constant_value"], p["k1__k2__length_scale"], p["k2__noise_level"])
                rows.append(dict(m=m, hyper=hyper, lml=gp.log_marginal_likelihood_value_, cond=np.linalg.cond(gp.kernel_(X)),
                                 traj=fr.scan(X, Y, *hyper, 1e-10, traj), grid=fr.scan(X, Y, *hyper, 1e-10, grid, surrogate=False)))
    finally:
        np.random.set_state(state)
    return rows


def test_letter_s_facts_from_sklearn_alone():
    from gaussian_process_transportation_amd.gaussian_process_transportation_diffeomorphic import select_trial
    rows = letter_s_table()
    for r in rows:
        print(f"m={r['m']:6.2f} ls={np.round(r['hyper'][1], 2)} lml={r['lml']:8.2f} min_det={float(r['traj']['min_det']):+.3f} "
              f"folds {r['traj']['n_fold']:3d} (grid {r['grid']['n_fold']:3d}) error={float(r['traj']['err_sum']):7.1f} "
              f"min|det| {float(np.abs(r['traj']['det']).min()):.1e} (grid {float(np.abs(r['grid']['det']).min()):.1e}) cond={r['cond']:.1e}")
    # every det the counts below rely on is at least 1000 x the tolerance the device scan is held to: no sign is in doubt, no
    # point is excluded from a count
    for r in rows:
        assert float(np.abs(r["traj"]["det"]).min()) >= 1000 * DET_TOLERANCE and float(np.abs(r["grid"]["det"]).min()) >= 1000 * DET_TOLERANCE
        assert r["cond"] <= 2e5
    ms = np.round(CANDIDATES, 2)
    assert [m for m, r in zip(ms, rows) if r["traj"]["n_fold"] == 0] == [3.34, 4.31]
    assert [m for m, r in zip(ms, rows) if r["grid"]["n_fold"] == 0] == [4.31]
    assert [r["traj"]["n_fold"] for r in rows] == [10, 6, 0, 0, 12, 15, 18, 21, 21, 21]
    table = dict(lml=[r["lml"] for r in rows], error=[float(r["traj"]["err_sum"]) for r in rows], min_det=[float(r["traj"]["min_det"]) for r in rows],
                 n_fold=[r["traj"]["n_fold"] for r in rows], status=[0] * len(rows))
    best, fell_back = select_trial("error", **table)
    assert ms[best] == 2.00 and rows[best]["traj"]["n_fold"] == 10 and not fell_back
    best, fell_back = select_trial("fold_free", **table)
    assert ms[best] == 4.31 and not fell_back
    table["n_fold"] = [r["grid"]["n_fold"] for r in rows]
    assert ms[select_trial("fold_free", **table)[0]] == 4.31
    assert abs(float(rows[-1]["traj"]["err_sum"]) - 332.37) < 0.01          # the unconstrained fit: the fixture's theta


# ------------------------------------------------------------------------------------------------------- 4. the selection rules
def test_selection_rules_on_hand_made_tables():
    from gaussian_process_transportation_amd.gaussian_process_transportation_diffeomorphic import select_trial
    OK, NOT_PD, nan = 0, -2, np.nan
    # fold_free: the highest LML among n_fold == 0, the first on ties; a higher LML that folds does not count
    t = dict(lml=[5.0, 1.0, 3.0, 3.0, 9.0], error=[1.0, 1.0, 1.0, 1.0, 1.0], min_det=[-1, 0.1, 0.2, 0.3, -0.5], n_fold=[4, 0, 0, 0, 7], status=[OK] * 5)
    assert select_trial("fold_free", **t) == (2, False)
    # error: the lowest, the first on ties
    t["error"] = [3.0, 2.0, 5.0, 2.0, 2.5]
    assert select_trial("error", **t) == (1, False)
    # no fold-free candidate: the largest min_det, flagged
    t["n_fold"] = [4, 1, 2, 3, 7]
    assert select_trial("fold_free", **t) == (3, True)
    # a candidate that is not PD takes no part, whatever its (untouched) numbers say
    t = dict(lml=[nan, 1.0, 2.0], error=[nan, 4.0, 3.0], min_det=[nan, 0.5, -0.1], n_fold=[-1, 0, 2], status=[NOT_PD, OK, OK])
    assert select_trial("fold_free", **t) == (1, False) and select_trial("error", **t) == (2, False)
    t["n_fold"] = [0, 3, 2]
    t["min_det"] = [9.0, -0.5, -0.1]
    assert select_trial("fold_free", **t) == (2, True)
    # a NaN error with surrogate_status set: out of the error criterion, still in the fold-free one
    t = dict(lml=[1.0, 2.0, 0.5], error=[nan, 7.0, 8.0], min_det=[0.1, 0.2, 0.3], n_fold=[0, 0, 0], status=[OK] * 3, surrogate_status=[NOT_PD, OK, OK])
    assert select_trial("error", **t) == (1, False) and select_trial("fold_free", **t) == (1, False)
    t["error"], t["surrogate_status"] = [1.0, 7.0, 8.0], [NOT_PD, OK, OK]                   # a stale number does not count either
    assert select_trial("error", **t) == (1, False)
    with pytest.raises(np.linalg.LinAlgError):
        select_trial("error", lml=[1.0], error=[nan], min_det=[0.1], n_fold=[0], status=[OK], surrogate_status=[NOT_PD])
    with pytest.raises(np.linalg.LinAlgError):
        select_trial("fold_free", lml=[1.0], error=[1.0], min_det=[0.1], n_fold=[0], status=[NOT_PD])
    with pytest.raises(ValueError, match="criterion"):
        select_trial("best", lml=[1.0], error=[1.0], min_det=[0.1], n_fold=[0], status=[OK])
