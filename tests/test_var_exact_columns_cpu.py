"""The designs of tests/test_var_exact_columns.py on the CPU (no GPU): the conditions on the INPUTS under which that file's
assertions mean what they say, and a numpy restatement of its calibration and product checks inside the same bounds.

  * wide lattices (D >= 4): every coordinate separates a pair of sites that agree in all others (var_exact_designs.separation),
    sites are distinct and exact in fp32;
  * the exactness conditions of the bit-for-bit tests, per element type (Design.check_exact through Design.expected) and per
    task of the multi-task model (var_exact_designs.expected_task);
  * derivative columns: every source off the query's site generates exactly 0 (the type's underflow threshold), the queries'
    coordinates are numbers of the type, and one dropped or doubled (i, k) term changes every checked output by at least 16 bounds -
    which F1's w in [-8, 8] does NOT meet in fp32 at N = 1300 (asserted: that is why fp32 takes the |w| = 1 design);
  * the restatement (var_exact_designs.restate_columns: the columns as k_var generates them, in the model's type, numpy's
    exp) goes through ColumnOutput.check exactly as the device's outputs do."""
import functools

import numpy as np
import pytest

from tests import var_exact_designs as vx

P = 256                                                    # workgroups of the plans looked at here: the MI355X's compute units
KINDS = {0: "rbf", 2: "matern32", 3: "matern52"}
DTYPES = {"fp64": np.float64, "fp32": np.float32}
WIDE_D = (4, 8, 9, 15)
COLUMN_D = (2, 3, 4, 6, 8, 12)
TASK_C = (1.0, 2.0, 0.25)


def padded(N):
    return -(-N // 512) * 512


def wide_designs(N, D, pow2):
    kw = dict(D=D, pow2=pow2)
    return {"F1": vx.f1(N, **kw), "G1": vx.f2(N, 1, **kw), "G7i": vx.f2(N, 7, interleaved=True, **kw),
            "c8": vx.f2(N, -(-N // 8), offsets=(0, 1, 2), **kw), "c8i": vx.f2(N, -(-N // 8), interleaved=True, offsets=(0, 1, 2), **kw)}


# ---- part A: wide layouts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("N", [512, 1300])
@pytest.mark.parametrize("D", WIDE_D)
def test_wide_lattices_separate_every_coordinate(D, N, pow2):
    for which, d in wide_designs(N, D, pow2).items():
        assert d.X.shape == (N, D) and d.coords.min() >= vx.SPACING and d.coords.max() < 2 ** 24
        assert len({tuple(x) for x in d.coords.tolist()}) == d.n_sites
        assert np.array_equal(d.coords.astype(np.float32).astype(np.float64), d.coords)
        if pow2:
            assert np.all(np.frexp(d.coords)[0] == 0.5)
        occ_occ, occ_any = vx.separation(d.coords, d.n_occupied)
        assert all(occ_any), (which, occ_any)
        if d.n_occupied >= D + 1:
            assert all(occ_occ), (which, occ_occ)
        else:
            assert which in ("G1", "G7i") and d.n_sites - d.n_occupied >= D      # the star sits on empty sites, which the batches visit
        # exactness: fp64 for the designs the fp64 cases use, fp32 for the fp32-safe ones
        if which in ("F1", "G1", "G7i"):
            d.expected(np.float64)
        if which in ("F1", "c8", "c8i"):
            assert np.array_equal(d.expected(np.float32).astype(np.float64), d.expected(np.float64))
            W = d.W()
            assert np.array_equal(W.astype(np.float32).astype(np.float64), W)


def test_narrow_lattices_are_what_they_were():
    """the D <= 3 lattice of the existing bit-for-bit tests is untouched by the wide one"""
    c = vx.lattice(30, 3)
    assert np.array_equal(c[:5], 1024.0 * np.array([[1, 1, 1], [2, 1, 1], [3, 1, 1], [4, 1, 1], [1, 2, 1]]))
    assert np.array_equal(vx.lattice(5, 1, pow2=True)[:, 0], 1024.0 * 2.0 ** np.arange(5))


# ---- part A: multi-task -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("N", [512, 1300])
@pytest.mark.parametrize("D", [3, 6])
def test_multitask_designs_meet_their_exactness_conditions(D, N, dname):
    dtype = DTYPES[dname]
    ds = [vx.f1(N, D, pow2=dtype == np.float32, seed=1000 * (t + 1) + N) for t in range(3)]
    assert all(np.array_equal(d.X, ds[0].X) for d in ds)                    # one set of inducing points
    assert not np.array_equal(ds[0].wint, ds[1].wint) and not np.array_equal(ds[1].wint, ds[2].wint)
    for d, c in zip(ds, TASK_C):
        want = vx.expected_task(d, c, 0.0, dtype)                           # asserts the conditions
        assert want.dtype == dtype and want[-1] == dtype(c) and np.all(want[:d.n_occupied] < want[-1]) and np.all(want > 0)
        # a task that read its neighbour's factor, or its neighbour's outputscale, would return other numbers at most sites
        other = vx.expected_task(ds[(ds.index(d) + 1) % 3], c, 0.0, dtype)
        assert np.mean(other[:d.n_occupied] != want[:d.n_occupied]) > 0.9
        Wc = d.W() * c
        assert np.array_equal(Wc.astype(dtype).astype(np.float64), Wc)


# ---- part B: derivative columns -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def column_design(N, D, dname, seed=None, c_t=1.0):
    return vx.column_design(N, D, DTYPES[dname], seed, c_t)


def all_batches(D, nbi, ntask, n_all):
    out = {}
    for flags in vx.REQUESTS:
        out[vx.request_name(flags)] = vx.column_batches(D, flags, nbi, ntask, P, n_all)
    return out


COLUMN_CASES = [(dn, kt, D, 1300) for dn in DTYPES for kt in KINDS for D in COLUMN_D] + [("fp64", 0, 3, 512), ("fp32", 2, 8, 512)]


@pytest.mark.parametrize("dname,kt,D,N", COLUMN_CASES)
def test_derivative_designs_and_restatement(dname, kt, D, N):
    dtype = DTYPES[dname]
    d = column_design(N, D, dname)
    nbi = padded(N) // 512
    total = d.n_sites + 1
    qsite = vx.column_sites(d, total)                        # every site once
    assert sorted(qsite.tolist()) == list(range(-1, d.n_sites))
    delta = vx.deltas(D, total)
    mags = np.abs(delta)
    assert np.all(mags == mags[0]) and len(set(mags[0].tolist())) == D and all((delta[:, k] > 0).any() and (delta[:, k] < 0).any() for k in range(D))
    assert np.all(np.frexp(mags[0] * 128)[1] <= 8) and np.all(mags[0] * 128 == np.rint(mags[0] * 128))       # dyadic
    vx.check_zero_off_site(d, kt, dtype, delta)
    depth = max(dp for _, dp in all_batches(D, nbi, 1, total).values())
    flags = dict(var=True, Jvar=True, dvar=True)
    cos = vx.column_outputs(d, kt, dtype, qsite, delta, flags)
    es = sorted({int(e) for co in cos.values() for e in np.unique(co.e)})
    cal = {(e, j): vx.restate_columns(d, kt, dtype, qsite, delta, flags, (e, j)) for e in es for j in range(nbi)}
    out = vx.restate_columns(d, kt, dtype, qsite, delta, flags, d.W())
    _, minw = vx.site_sums(d, qsite)
    for k, co in cos.items():
        # the calibrated s2 is within a factor 8 of the prior term
        b2, _ = co.calibrated({ej: c[k] for ej, c in cal.items()}, 0)
        s2c = np.abs(b2[co.occ]).astype(np.float64) * 4.0 ** co.e[co.occ]
        ref = float(co.prior) if co.subtract else 1.0
        assert np.all(s2c <= ref) and np.all(s2c >= ref / 8)
        r_op, r_pr = co.check({ej: c[k] for ej, c in cal.items()}, out[k], depth)
        disc = co.discrimination(minw, co.last["bound"])
        print(f"{d.name} {KINDS[kt]} {dname} {k}: depth {depth}, operand error / bound {r_op:.3f}, product error / bound {r_pr:.3f}, "
              f"smallest change of one term / (16 bounds) {disc:.2f}")
        assert r_op <= 1.0 and r_pr <= 1.0
        assert disc >= 1.0, "a dropped or doubled term could hide inside the bound: replace the design"


def test_f1_fails_the_discrimination_condition_in_fp32():
    """F1's w in [-8, 8]: a term with |w| = 1 is 1 / 64 of one with |w| = 8, and at N = 1300 the smallest change falls below 16 bounds
    in fp32 - the reason the fp32 cases take |w| = 1.  (In fp64 F1 has eight orders of magnitude to spare.)"""
    N, D, kt = 1300, 3, 0
    for dtype, fails in ((np.float32, True), (np.float64, False)):
        d = vx.f1(N, D, spacing=128, e_shift=1)
        qsite = vx.column_sites(d, d.n_sites + 1)
        delta = vx.deltas(D, len(qsite))
        flags = dict(Jvar=True)
        co = vx.column_outputs(d, kt, dtype, qsite, delta, flags)["Jvar"]
        es = [int(e) for e in np.unique(co.e)]
        cal = {(e, j): vx.restate_columns(d, kt, dtype, qsite, delta, flags, (e, j))["Jvar"] for e in es for j in range(3)}
        co.check(cal, vx.restate_columns(d, kt, dtype, qsite, delta, flags, d.W())["Jvar"], 82)
        disc = co.discrimination(vx.site_sums(d, qsite)[1], co.last["bound"])
        print(f"F1 N = 1300 {dtype.__name__}: smallest change / (16 bounds) {disc:.3g}")
        assert (disc < 1.0) == fails


@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("D", [3, 6])
def test_multitask_derivative_designs_and_restatement(D, dname):
    dtype, N, kt = DTYPES[dname], 1300, 0
    ds = [column_design(N, D, dname, 1000 * (t + 1) + N, TASK_C[t]) for t in range(3)]
    total = ds[0].n_sites + 1
    qsite = vx.column_sites(ds[0], total)
    delta = vx.deltas(D, total)
    flags = dict(var=True, Jvar=True)
    depth = max(vx.column_batches(D, f, 3, 3, P, total)[1] for f in (dict(Jvar=True), flags))
    for d, c in zip(ds, TASK_C):
        vx.check_zero_off_site(d, kt, dtype, delta)
        cos = vx.column_outputs(d, kt, dtype, qsite, delta, flags, c_t=c, noise=0.0)
        es = sorted({int(e) for co in cos.values() for e in np.unique(co.e)})
        cal = {(e, j): vx.restate_columns(d, kt, dtype, qsite, delta, flags, (e, j), c_t=c, noise=0.0) for e in es for j in range(3)}
        out = vx.restate_columns(d, kt, dtype, qsite, delta, flags, d.W(), c_t=c, noise=0.0)
        _, minw = vx.site_sums(d, qsite, c)
        for k, co in cos.items():
            r_op, r_pr = co.check({ej: cl[k] for ej, cl in cal.items()}, out[k], depth)
            disc = co.discrimination(minw, co.last["bound"])
            print(f"{d.name} c = {c} {dname} {k}: operand {r_op:.3f}, product {r_pr:.3f}, discrimination {disc:.2f}")
            assert r_op <= 1.0 and r_pr <= 1.0 and disc >= 1.0


def test_calibration_factors_reach_every_block_of_every_source():
    """calibration_factor(N, e, j): lower triangular, one entry 2^e per column whose block k // 512 + j exists, in a row of that
    block; restate_columns' shortcut for it is the dense product"""
    N = 1300
    d = column_design(N, 3, "fp64")
    qsite = vx.column_sites(d, 200)
    delta = vx.deltas(3, 200)
    flags = dict(var=True, Jvar=True, dvar=True)
    for j in range(3):
        W = vx.calibration_factor(N, 2, j)
        assert not np.triu(W, 1).any() and set(np.unique(W).tolist()) <= {0.0, 4.0}
        rows, cols = np.nonzero(W)
        assert np.array_equal(rows // 512, cols // 512 + j) and np.array_equal(np.unique(cols), np.arange(N)[512 * (np.arange(N) // 512 + j) < N])
        a = vx.restate_columns(d, 0, np.float64, qsite, delta, flags, (2, j))
        b = vx.restate_columns(d, 0, np.float64, qsite, delta, flags, W)
        assert all(np.array_equal(a[k], b[k]) for k in a)


def test_operand_reference_is_the_kernel_of_the_oracle():
    """column_reference against the project's numpy Matern posterior pieces and the RBF closed form, in double: k and dk/dx at a few
    offsets (the reference the operand check stands on must itself be the right function)"""
    from tests.test_matern_derivatives import G0
    assert G0[1.5] == vx.G0[vx.KT_M32] and G0[2.5] == vx.G0[vx.KT_M52]
    delta = vx.deltas(3, 7)
    eps = 1e-6
    for kt in KINDS:
        k, dk = vx.column_reference(kt, delta)
        for d in range(3):
            step = np.zeros(3)
            step[d] = eps
            # d k(x, X) / d x_d at x = X + delta, by central differences of the reference's own k
            kp, _ = vx.column_reference(kt, delta + step)
            km, _ = vx.column_reference(kt, delta - step)
            assert np.allclose(((kp - km) / (2 * eps)).astype(np.float64), dk[:, d].astype(np.float64), rtol=1e-7, atol=1e-9)
        r = np.sqrt((delta ** 2).sum(axis=1))
        want = {0: np.exp(-r * r / 2), 2: (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r),
                3: (1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r)}[kt]
        assert np.allclose(k.astype(np.float64), want, rtol=1e-14)
