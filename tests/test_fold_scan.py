"""gpt_batch_fold_scan (csrc/gpt_fold_scan.hip) on the GPU: against the longdouble restatement at the shapes where it can go wrong,
its reductions against its own per-query arrays (exactly), its independence of the batch, the queries and the optional arrays
(bit for bit), the isolation of a member that is not positive definite, and its refusals.

Inputs, reference and the derivation of every tolerance: tests/fold_scan_cases.py (conditions asserted in test_fold_scan_cpu.py).
Each case prints `ratio <case> n=<n> <quantity> <gpu error / max(e_oracle, n 2^-53)>`; a ratio above 32 fails."""
import numpy as np
import pytest

from tests import fold_scan_cases as fc
from tests import fold_scan_restatement as fr

gpu = pytest.mark.gpu
LD = fc.LD


def run(s, members=None, per_query=True, surrogate=True, jitter=fc.JITTER):
    """The members of a case (default: all) through one call."""
    from gaussian_process_transportation_amd import _lib
    members = list(range(len(s["Xs"]))) if members is None else members
    shared = len(s["xqs"]) != len(s["Xs"])
    xq = s["xqs"][0] if shared else [s["xqs"][b] for b in members]
    return _lib.batch_fold_scan([s["Xs"][b] for b in members], [s["Ys"][b] for b in members], s["ls"][members], s["c"][members],
                                s["noise"][members], jitter, xq, surrogate=surrogate, per_query=per_query)


def check_reductions(got, b, M):
    """A member's five numbers against the call's own per-query arrays: exact."""
    det, err = got["det"][b], got["err"][b]
    if M == 0:
        assert (got["min_det"][b], got["argmin"][b], got["n_fold"][b], got["err_sum"][b], got["err_max"][b]) == (np.inf, -1, 0, 0.0, 0.0)
        return
    assert got["n_fold"][b] == int((det <= 0).sum())
    assert got["min_det"][b] == det.min() and got["argmin"][b] == int(np.argmin(det))      # np.argmin: the first index
    assert got["err_max"][b] == err.max()


@gpu
@pytest.mark.parametrize("cid", fc.CASES)
def test_scan_against_the_longdouble_restatement(cid):
    s = fc.case(cid)
    got = run(s)
    B = len(s["Xs"])
    assert got["status"].tolist() == [0] * B and got["surrogate_status"].tolist() == [0] * B
    bad = []
    for b in range(B):
        n, ref, e_o, M = len(s["Xs"][b]), s["ref"][b], s["e_oracle"][b], len(fc.queries_of(s, b))
        assert got["det"][b].shape == (M,) and got["z"][b].shape == (M, s["D"]) and got["err"][b].shape == (M,)
        check_reductions(got, b, M)
        if M == 0:
            continue
        floor = n * 2.0 ** -53
        for q in ("z", "err"):
            tol = fc.tolerance(e_o[q], n)
            assert tol <= fc.CAP
            e = fc.relerr(got[q][b], ref[q])
            print(f"ratio {cid} n={n} {q} {e / max(e_o[q], floor):.2f}   (gpu {e:.2e}, oracle {e_o[q]:.2e}, tol {tol:.2e})")
            if not e <= tol:
                bad.append((b, n, q, e, tol))
        tol_J = fc.tolerance(e_o["J"], n)
        bound = fc.det_bound(ref, tol_J)                   # absolute, per query
        d = np.abs(got["det"][b].astype(LD) - ref["det"]).astype(np.float64)
        worst = int(np.argmax(d / bound))
        print(f"ratio {cid} n={n} det {fc.FACTOR * d[worst] / bound[worst]:.2f}   (gpu {d[worst]:.2e} absolute, bound {bound[worst]:.2e}, "
              f"oracle J {e_o['J']:.2e})")
        if not np.all(d <= bound):
            bad.append((b, n, "det", d[worst], bound[worst]))
        # the counts agree with the reference wherever no reference det is within the bound of zero
        if np.all(np.abs(ref["det"]).astype(np.float64) > bound):
            assert got["n_fold"][b] == ref["n_fold"], (cid, b)
        err_abs = fc.tolerance(e_o["err"], n) * float(np.max(np.abs(ref["err"])))
        tol_sum = M * (err_abs + 2.0 ** -53 * float(ref["err_sum"]))
        ds = float(abs(LD(got["err_sum"][b]) - ref["err_sum"]))
        print(f"ratio {cid} n={n} err_sum {fc.FACTOR * ds / tol_sum:.2f}   (gpu {ds:.2e} absolute, bound {tol_sum:.2e})")
        if not ds <= tol_sum:
            bad.append((b, n, "err_sum", ds, tol_sum))
    assert not bad, (cid, bad)


@gpu
def test_reductions_and_queries_do_not_depend_on_their_surroundings():
    """Bit for bit: a member alone, at the other end of a batch of 7, with and without the per-query arrays, with and without the
    surrogate (det side); a query alone (M = 1) and inside the largest M; shared and ragged queries."""
    s = fc.case("sizes-D2-ard")
    full = run(s)
    lean = run(s, per_query=False)
    assert "det" not in lean
    plain = run(s, surrogate=False)
    assert np.all(np.isnan(plain["err_sum"])) and np.all(np.isnan(plain["err_max"])) and all(np.all(np.isnan(e)) for e in plain["err"])
    flipped = run(s, members=list(range(6, -1, -1)))
    for b in range(7):
        alone = run(s, members=[b])
        for q in ("min_det", "argmin", "n_fold", "err_sum", "err_max"):
            assert np.array_equal(full[q][b], lean[q][b]) and np.array_equal(full[q][b], alone[q][0]) and \
                np.array_equal(full[q][b], flipped[q][6 - b]), (b, q)
        for q in ("min_det", "argmin", "n_fold"):
            assert np.array_equal(full[q][b], plain[q][b]), (b, q)
        for q in ("det", "z", "err"):
            assert np.array_equal(full[q][b], alone[q][0]) and np.array_equal(full[q][b], flipped[q][6 - b]), (b, q)
        assert np.array_equal(full["det"][b], plain["det"][b]) and np.array_equal(full["z"][b], plain["z"][b])
    # one query of the largest set, alone
    from gaussian_process_transportation_amd import _lib
    b = 5
    for i in (0, 63, 64, 192):
        one = _lib.batch_fold_scan([s["Xs"][b]], [s["Ys"][b]], s["ls"][[b]], s["c"][[b]], s["noise"][[b]], fc.JITTER, s["xqs"][b][i:i + 1],
                                   per_query=True)
        for q in ("det", "z", "err"):
            assert np.array_equal(one[q][0][0], full[q][b][i]), (i, q)
        assert one["min_det"][0] == full["det"][b][i] and one["argmin"][0] == 0 and one["err_sum"][0] == full["err"][b][i]
    # the same queries shared by both members, and handed to each as its own
    s2 = fc.case("shared-B2")
    shared = run(s2)
    ragged = _lib.batch_fold_scan(s2["Xs"], s2["Ys"], s2["ls"], s2["c"], s2["noise"], fc.JITTER, [s2["xqs"][0], s2["xqs"][0]], per_query=True)
    for q in ("min_det", "argmin", "n_fold", "err_sum", "err_max"):
        assert np.array_equal(shared[q], ragged[q]), q
    for q in ("det", "z", "err"):
        assert all(np.array_equal(shared[q][b], ragged[q][b]) for b in range(2)), q


@gpu
def test_ties_take_the_first_index():
    """Queries repeated across tiles: the minimum is attained several times, argmin is the first of them."""
    s = fc.case("shared-B1")
    xq = np.tile(s["xqs"][0][:5], (40, 1))                 # 200 queries, period 5: four tiles
    from gaussian_process_transportation_amd import _lib
    got = _lib.batch_fold_scan(s["Xs"], s["Ys"], s["ls"], s["c"], s["noise"], fc.JITTER, xq, per_query=True)
    det = got["det"][0]
    assert np.array_equal(det, np.tile(det[:5], 40))
    assert got["argmin"][0] == int(np.argmin(det[:5])) and got["min_det"][0] == det.min()
    assert got["n_fold"][0] == 40 * int((det[:5] <= 0).sum())


def _isolation_batch():
    """Members 0 and 3: ordinary.  Member 1: rows 0 and 1 identical, c = 1, noise 0 (jitter 0 for the call): the second pivot of
    its source matrix is 1 - 1 * 1 = 0.  Member 2: distinct sources, but rows 0 and 1 are displaced onto one target point (exact
    sums), so the second pivot of the surrogate's matrix alone is 0."""
    rng = np.random.default_rng(11)
    Xs, Ys, ls, c, noise = map(list, zip(*(fc.draw_model(rng, n, 2, 2) for n in (12, 6, 6, 40))))
    Xs[1][1] = Xs[1][0]
    Xs[2][0], Ys[2][0] = [0.25, 0.5], [0.25, 0.0]
    Xs[2][1], Ys[2][1] = [0.75, 0.5], [-0.25, 0.0]
    c[1] = c[2] = 1.0
    noise[1] = noise[2] = 0.0
    xqs = [rng.uniform(-0.1, 1.1, (m, 2)) for m in (5, 70, 65, 9)]
    return Xs, Ys, np.array(ls), np.array(c), np.array(noise), xqs


@gpu
def test_a_member_that_is_not_positive_definite_is_isolated():
    from gaussian_process_transportation_amd import _lib
    Xs, Ys, ls, c, noise, xqs = _isolation_batch()

    def call(members):
        return _lib.batch_fold_scan([Xs[b] for b in members], [Ys[b] for b in members], ls[members], c[members], noise[members], 0.0,
                                    [xqs[b] for b in members], per_query=True)
    got = call([0, 1, 2, 3])
    assert got["status"].tolist() == [0, _lib.GPT_E_NOT_PD, 0, 0]
    assert got["surrogate_status"][[0, 2, 3]].tolist() == [0, _lib.GPT_E_NOT_PD, 0]
    # member 1: every output as the wrapper initialised it (NaN, -1)
    assert np.isnan(got["min_det"][1]) and got["argmin"][1] == -1 and got["n_fold"][1] == -1 and np.isnan(got["err_sum"][1]) and np.isnan(got["err_max"][1])
    assert np.all(np.isnan(got["det"][1])) and np.all(np.isnan(got["z"][1])) and np.all(np.isnan(got["err"][1]))
    # member 2: the err outputs untouched, the det side computed and consistent
    assert np.isnan(got["err_sum"][2]) and np.isnan(got["err_max"][2]) and np.all(np.isnan(got["err"][2]))
    assert np.all(np.isfinite(got["det"][2])) and np.all(np.isfinite(got["z"][2]))
    assert got["min_det"][2] == got["det"][2].min() and got["argmin"][2] == int(np.argmin(got["det"][2])) and got["n_fold"][2] == int((got["det"][2] <= 0).sum())
    ref = fr.scan(Xs[2], Ys[2], c[2], ls[2], noise[2], 0.0, xqs[2])
    assert ref["surrogate_status"] == fr.NOT_PD and fc.relerr(got["det"][2], ref["det"]) <= 1e-9
    # the neighbours: bit for bit their solo results
    for b in (0, 3):
        alone = call([b])
        assert alone["status"].tolist() == [0] and alone["surrogate_status"].tolist() == [0]
        for q in ("min_det", "argmin", "n_fold", "err_sum", "err_max"):
            assert np.array_equal(got[q][b], alone[q][0]), (b, q)
        for q in ("det", "z", "err"):
            assert np.array_equal(got[q][b], alone[q][0]) and np.all(np.isfinite(got[q][b])), (b, q)


@gpu
def test_refusals_name_the_limit():
    from gaussian_process_transportation_amd import _lib
    rng = np.random.default_rng(3)
    X, Y, ls, c, noise = fc.draw_model(rng, 10, 2, 2)
    xq = rng.uniform(0, 1, (5, 2))
    nb = np.array([0, 10], dtype=np.int64)

    def packed(X=X, Y=Y, nb=nb, ls=ls, xq=xq, q_begin=None, kernel_type=0):
        return _lib.batch_fold_scan_packed(X, Y, nb, ls[None, :], [c], [noise], 1e-10, xq, q_begin, kernel_type=kernel_type)
    assert packed()["status"].tolist() == [0]
    X4 = rng.uniform(0, 1, (10, 4))
    with pytest.raises(ValueError, match=r"D must be 1 \.\. 3"):
        packed(X=X4, Y=X4, ls=np.ones(4), xq=np.zeros((5, 4)))
    with pytest.raises(ValueError, match=r"Y must be of shape \(n_b, D\)"):
        packed(Y=np.zeros((10, 1)))
    with pytest.raises(ValueError, match="RBF only"):
        packed(kernel_type=2)
    X129 = rng.uniform(0, 1, (129, 2))
    with pytest.raises(ValueError, match=r"1 <= n_b <= 128"):
        packed(X=X129, Y=0.1 * X129, nb=np.array([0, 129], dtype=np.int64))
    with pytest.raises(ValueError, match=r"1 \.\. 128 points"):
        _lib.batch_fold_scan([X129], [0.1 * X129], ls[None, :], [c], [noise], 1e-10, xq)
    bad = xq.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="Xq contains NaN"):
        packed(xq=bad)
    X2, Y2 = np.concatenate([X, X]), np.concatenate([Y, Y])
    with pytest.raises(ValueError, match="q_begin must not decrease"):
        _lib.batch_fold_scan_packed(X2, Y2, np.array([0, 10, 20], dtype=np.int64), np.stack([ls, ls]), [c, c], [noise, noise], 1e-10, xq,
                                    np.array([0, 4, 3], dtype=np.int64))
