"""k_var, k_var_combine and k_var_finalize on operands whose answer is known - the launches tests/test_var_exact.py leaves out:
wide layouts (D >= 4), the stacked factors of a multi-task model, and every launch with derivative columns.  Designs, references
and bounds are in tests/var_exact_designs.py; tests/test_var_exact_columns_cpu.py asserts the conditions on the inputs.

A. BIT FOR BIT (the k* column alone, queries on sites, np.array_equal against Design.expected, as check_kvar of test_var_exact.py):
   * wide layouts: D = 4, 8 (source rows of 8) and 9, 15 (rows of 16), N = 512 and 1300, both element types, all four kernel
     types, on a lattice whose every coordinate separates a pair of sites (var_exact_designs.lattice: without that a coordinate
     the wide generating sweep dropped, or read from another row of its query image, would change nothing).  The Matern models
     take the `pow2` lattice, and so does every fp32 model: the rows-of-16 sweep forms fma(x, 1/sqrt 2, -q'), whose value at a
     coincident site is the rounding error of x / sqrt 2 - nothing in fp64 (h ~ 1e-24 under an exp), but 1e-4 at x = 3072 in
     fp32, where exp(-h) then falls below 1; a power of two times 1/sqrt 2 is exact.  (The D <= 3 sweep shows the same in fp32
     once s2 is large enough to carry it: a task with outputscale 2 on the plain lattice returned one ulp more at the site with
     two coordinates of 9216, where k* is 1 - 2^-23.  test_var_exact.py's fp32 cases have s2 < 1/4 and do not see it.  It is the
     property DESIGN.md describes for the Matern kernels, not a wrong term; the fp32 multi-task designs take the pow2 lattice too.)
   * multi-task: a gpt_fit_svgp model of T = 3 tasks (outputscales 1, 2, 1/4, Sigma = noise I) whose three factor slots take three
     different F1 designs through gpt_debug_set_task_inverse_factor.  k_var_finalize restated: task t reads hdr[16 + t] = c_t, the
     model's own noise is 0 (Sigma went into the fit, not into the prediction), the slot holds c_t W_t, so
     var[m, t] = fl(c_t - c_t^2 s2_t) (var_exact_designs.expected_task asserts the exactness conditions per task).

B. DERIVATIVE COLUMNS, calibrated.  A derivative column is c g(r) u_d: 0 on a site, inexact off it.  Sources sit on sites, one
   per site (F1; fp32: |w| = 1), queries at site + delta with |delta_d| distinct dyadic numbers per dimension and signs that vary.
   Every source off the query's site is beyond the type's underflow distance: its columns are exactly 0.  So a query near site g
   (source k) has  V[i, m, col] = W[i, k] beta[m, col],  one product per row, with beta the number k_var generated for (k, col).
   beta is NOT one number for all rows: a column block whose sweeps the plan shares out among workgroups (every tail) is generated
   once per workgroup, into that workgroup's scratch image, by whichever generating path its item takes (the batched opening, the
   diagonal tile, the fill inside the MFMA loop), and the paths need not round alike - x / sqrt 2 - q / sqrt 2 with the product
   fused into the subtraction or not differs by |x| u / |delta_d| relative, 1e-11 at |x| = 4e4 in fp64.  (Measured: with ONE
   calibrated beta per column the fp64 D = 2 design missed the product bound 600-fold at one query per site, and only there.)
   What holds is: all 512 rows of an i-block read the same fragments.  So  s2 = sum_j beta_j^2 S_(g, j),  j the i-block above
   the source's own, S_(g, j) = sum of W[i, k]^2 over that block's rows: exact integers times a power of two (site_sums).
   * calibration: the same handle, queries and request with W = 2^e at ONE row of block j in every column (calibration_factor;
     j = 0: 2^e I), for every j.  Then V = 2^e beta_j exactly, one non-zero square per column:
     s2_cal = fl(beta_j^2) 4^e, and the output is fl(prior - s2_cal) (dvar: -2 fl(beta_0 beta_d) 4^e, no subtraction).  The host
     reads beta_j^2 back in longdouble; its relative error is 2 u_cal = u + u |output_cal| / s2_cal (the square, the final
     subtraction).  e is chosen per element with 4^e beta^2 in (0.225, 0.9] prior: within a factor 8 of the prior term and
     below it (var is clamped at 0), so 2 u_cal <= 4.5 u.
   * operand check: calibrated beta^2 against the longdouble c g(|delta|) delta_d / l^2 (k for the k* column; c = l = 1).  Bound
     (var_exact_designs.operand_bound, first order, u the unit roundoff of the type, x the largest coordinate):
       - coordinates: d'_d = fl(x / sqrt 2) - fl(q / sqrt 2), two roundings of |x| / sqrt 2 against |delta_d| / sqrt 2:
         eps_d = 2 u |x| / |delta_d|;
       - h = sum d'^2: sum_d delta_d^2 eps_d from the coordinates and (D + 2) u h from its own products and fma;
       - RBF: the exponent is -h (ln c = 0).  Matern: t = sqrt(nu') sqrt(2 h), dt = t (dh / 2h + 4 u) (sqrt, constant, product);
         prefactors 3 (exact), (5/3)(1 + t): dt / (1 + t) + 3 u, 1 + t: dt / (1 + t) + u, 1 + t + t^2 / 3: dt (1 + 2t/3) / pre + 5 u,
         one more u for prefactor times exponential;
       - the exp: 3.5e-16 relative (gpt_exp.h, table exp) in fp64; fp32: 2 u |arg| (log2 e and its product) + 2 u (v_exp_f32, 1 ulp);
       - the column: kv (sqrt 2 / l) d'_d: 3 u + eps_d; the k* column is kv itself.
     beta^2 takes twice the column's bound, beta_0 beta_d the sum of the two, plus 2 u_cal.  This catches a wrong column,
     dimension, sign (dvar), kernel function (k for g), or length-scale.
   * product check: with the design's W every output must be prior - sum_j calibrated(beta_j^2) S_(g, j) (dvar: -2 sum_j
     calibrated(beta_0 beta_d)_j S_(g, j)) within  (2 u_prod + gamma_(depth + 1) + 2 u_cal) s2 + u |output|, every beta_j against the
     reference too:  V_i = fl(W beta) (u_prod each, twice in a square), the
     squares (one rounding each: the + 1) are added along a chain of at most `depth` additions, the final subtraction rounds
     once.  depth, read off the kernels: a lane adds 16 squares per sweep (4 row tiles x 4 elements of gpt_kvar.h's fold) over the
     nbi sweeps of its block, two shuffle additions (lanes + 16, + 32), the 8 waves' sums in a row, then k_var_finalize adds the
     block's slots in order - 1 for a block of a whole round, up to 8 nbi where sweeps were cut (k_var_combine writes 8 per cut
     sweep; inside it the chain is 4 + 2 + 4, shorter than a whole sweep's): depth = 16 nbi + 2 + 8 + slots, slots the longest
     range of the launch's plan (82 at nbi = 3, 34 at nbi = 1; the same for every launch kind).
   * discrimination (CPU file): one dropped or doubled (i, k) term changes every checked output by at least 16 bounds.
   * equalities: GPT_VAR_DIAG_HALF 0 / 1 bit-equal in fp64; a query ON a site returns Jvar = prior, dvar = 0 and the design's exact
     var; the origin and empty sites return the priors (sites with power-of-two coordinates: exact scaled coordinates).

Worst error / bound per launch kind is printed (DESIGN.md quotes a run)."""
import functools

import numpy as np
import pytest

from tests import var_exact_designs as vx
from tests.test_var_exact import check_kvar, model, padded, small_batches, workgroups

pytestmark = pytest.mark.gpu

KIND_NAMES = ("rbf", "matern12", "matern32", "matern52")
TASK_C = (1.0, 2.0, 0.25)


def np_dtype(f32):
    return np.float32 if f32 else np.float64


# ---- A.1 wide layouts ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def wide_design(N, which, D, pow2):
    kw = dict(D=D, pow2=pow2)
    return {"F1": lambda: vx.f1(N, **kw), "G1": lambda: vx.f2(N, 1, **kw), "G7i": lambda: vx.f2(N, 7, interleaved=True, **kw),
            "c8": lambda: vx.f2(N, -(-N // 8), offsets=(0, 1, 2), **kw),
            "c8i": lambda: vx.f2(N, -(-N // 8), interleaved=True, offsets=(0, 1, 2), **kw)}[which]()


def feature_batch(feature, nbi, ntask=1):
    got = vx.pick_queries(feature, 1, nbi, ntask, workgroups())
    if got is None:
        pytest.fail(f"no candidate batch size has the plan feature {feature} at nbi = {nbi}, {ntask} task(s) on {workgroups()} workgroups")
    return got[0]


@pytest.mark.parametrize("N", [512, 1300])
@pytest.mark.parametrize("D", [4, 8, 9, 15])
@pytest.mark.parametrize("kind", range(4), ids=KIND_NAMES)
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_wide_layouts_bit_for_bit(f32, kind, D, N, monkeypatch):
    nbi = padded(N) // 512
    Ms = [feature_batch(f, nbi) for f in ("tail_cut", "rounds_and_tail")]
    for which in (("F1", "c8", "c8i") if f32 else ("F1", "G1", "G7i")):
        d = wide_design(N, which, D, kind != 0 or f32)
        h = model(d, kind, f32)
        for qsite in small_batches(d) + [vx.cycle_sites(d, M, 37) for M in Ms]:
            check_kvar(h, d, qsite, monkeypatch, np_dtype(f32))
        h.close()


# ---- multi-task models ----------------------------------------------------------------------------------------------------------------
def task_seed(t, N):
    return 1000 * (t + 1) + N


def svgp_model(ds, f32):
    """a gpt_fit_svgp model on the designs' shared sites (K_uu + Sigma = (c_t + noise) I), every task's slot then holding its design"""
    from gaussian_process_transportation_amd import _lib
    N, D = ds[0].N, ds[0].D
    h = _lib.Handle(0)
    y = np.cos(np.arange(3 * N, dtype=np.float64)).reshape(3, N)
    Sigma = np.ascontiguousarray(np.broadcast_to(vx.NOISE * np.eye(N), (3, N, N)))
    h.fit_svgp(ds[0].X, y, Sigma, np.ones(D), np.array(TASK_C), 0.0, _lib.GPT_F32 if f32 else _lib.GPT_F64)
    assert h.model_info() == (3, 1 if f32 else 0)
    return h


def inject_tasks(h, Ws):
    for t, W in enumerate(Ws):
        h.debug_set_task_inverse_factor(t, W)


@pytest.mark.parametrize("N", [512, 1300])
@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_multitask_bit_for_bit(f32, D, N):
    from gaussian_process_transportation_amd import _lib
    dtype = np_dtype(f32)
    ds = [vx.f1(N, D, pow2=f32, seed=task_seed(t, N)) for t in range(3)]
    want = [vx.expected_task(d, c, 0.0, dtype) for d, c in zip(ds, TASK_C)]
    h = svgp_model(ds, f32)
    with pytest.raises(ValueError):
        h.debug_set_task_inverse_factor(3, ds[0].W())           # no such task
    with pytest.raises(_lib.GptError):
        h.debug_set_inverse_factor(ds[0].W())                   # the single-task hook keeps refusing a multi-task model
    inject_tasks(h, [d.W() for d in ds])
    d = ds[0]
    for qsite in small_batches(d) + [vx.cycle_sites(d, feature_batch("rounds_and_tail", padded(N) // 512, 3), 37)]:
        got = h.predict_all(d.queries(qsite), var=True)["var"]
        assert got.dtype == dtype and got.shape == (len(qsite), 3)
        for t in range(3):
            assert np.array_equal(got[:, t], want[t][qsite]), f"task {t}, M = {len(qsite)}\n" + vx.describe_wrong(ds[t], qsite, got[:, t], want[t][qsite])
    # one slot rewritten alone: the other two keep their factors
    inject_tasks(h, [ds[0].W(), ds[0].W(), ds[2].W()])
    qsite = d.site.copy()
    got = h.predict_all(d.queries(qsite), var=True)["var"]
    assert np.array_equal(got[:, 0], want[0][qsite]) and np.array_equal(got[:, 2], want[2][qsite])
    assert np.array_equal(got[:, 1], vx.expected_task(ds[0], TASK_C[1], 0.0, dtype)[qsite])
    h.close()


def test_task_hook_on_a_single_task_model_is_the_old_hook(monkeypatch):
    d = vx.f1(512)
    h = model(d)
    h.debug_set_task_inverse_factor(0, d.W())
    assert np.array_equal(np.tril(h.export_inverse_factor()), d.W())
    check_kvar(h, d, d.site, monkeypatch)
    with pytest.raises(ValueError):
        h.debug_set_task_inverse_factor(1, d.W())
    h.close()


# ---- B derivative columns ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def column_design(N, D, f32, seed=None, c_t=1.0):
    return vx.column_design(N, D, np_dtype(f32), seed, c_t)


def column_model(d, kt, f32):
    from gaussian_process_transportation_amd import _lib
    h = _lib.Handle(0)
    if f32:
        h.set_dtype(_lib.GPT_F32)
    h.set_matern_derivatives(True)
    Y = np.cos(np.arange(2 * d.N, dtype=np.float64)).reshape(d.N, 2)
    h.fit(d.X, Y, np.ones(d.D), vx.C, vx.NOISE, 0.0, kernel_type=kt)
    return h


def predict(h, Xq, flags):
    out = h.predict_all(Xq, **flags)
    return {k: out[k] for k in ("var", "Jvar", "dvar") if flags.get(k)}


def task_slice(a, key, t, ntask):
    """output `key` of task t: var (M, T) and Jvar (M, T, D) of a multi-task model"""
    return a if ntask == 1 else a[:, t]


def run_column_cases(h, ds, cs, kt, f32, requests, inject, monkeypatch, noise):
    """every request x batch of one handle: calibration runs (calibration_factor(N, e, j) in every slot) for the exponents e the
    elements need and every i-block offset j, then the designs' factors; returns {request name: (worst operand error / bound,
    worst product error / bound)}"""
    dtype, ntask, d0 = np_dtype(f32), len(ds), ds[0]
    N, D, nbi = d0.N, d0.D, padded(d0.N) // 512
    total = d0.n_sites + 1
    cases = []                                               # (flags, qsite, Xq, depth, [per task {key: ColumnOutput}])
    for flags in requests:
        Ms, _ = vx.column_batches(D, flags, nbi, ntask, workgroups(), total)
        from gaussian_process_transportation_amd import _lib
        for M in Ms:
            depth = vx.chain_depth(_lib.debug_var_plan(M * vx.cols_per_query(D, flags), nbi, ntask, workgroups()), nbi)
            qsite = vx.column_sites(d0, M)
            delta = vx.deltas(D, M)
            cos = [vx.column_outputs(d, kt, dtype, qsite, delta, flags, c_t=c, noise=noise) for d, c in zip(ds, cs)]
            cases.append((flags, qsite, d0.queries(qsite, delta), depth, cos))
    es = sorted({int(e) for case in cases for cos in case[4] for co in cos.values() for e in np.unique(co.e)})
    assert len(es) <= 8, es
    cal = {}
    for e in es:
        for j in range(nbi):
            inject(h, [vx.calibration_factor(N, e, j)] * ntask)
            cal[e, j] = [predict(h, Xq, flags) for flags, _, Xq, _, _ in cases]
    inject(h, [d.W() for d in ds])
    worst = {}
    for i, (flags, qsite, Xq, depth, cos) in enumerate(cases):
        out = predict(h, Xq, flags)
        if not f32:
            # the default took the HALF kernels where they exist; the plain ones must agree to the bit
            monkeypatch.setenv("GPT_VAR_DIAG_HALF", "0")
            plain = predict(h, Xq, flags)
            monkeypatch.delenv("GPT_VAR_DIAG_HALF")
            for k in out:
                assert np.array_equal(out[k], plain[k]), (k, flags)
        name = vx.request_name(flags)
        w = worst.setdefault(name, [0.0, 0.0])
        for t in range(ntask):
            for k, co in cos[t].items():
                assert out[k].dtype == dtype
                r_op, r_pr = co.check({ej: task_slice(c[i][k], k, t, ntask) for ej, c in cal.items()}, task_slice(out[k], k, t, ntask), depth)
                w[0], w[1] = max(w[0], r_op), max(w[1], r_pr)
                what = f"{ds[t].name} {KIND_NAMES[kt]} [{name}] M = {len(qsite)} task {t} {k}"
                assert r_op <= 1.0, f"{what}: the generated column is {r_op:.3g} of its bound away from c g(|delta|) delta_d"
                assert r_pr <= 1.0, f"{what}: |output - (prior - calibrated beta^2 S)| is {r_pr:.3g} of its bound"
    return worst


def single(h, Ws):
    h.debug_set_inverse_factor(Ws[0])


def on_site_equalities(h, d, kt, f32):
    """queries ON sites (power-of-two coordinates), on an empty site and at the origin, through the fused launches: every
    derivative column is exactly 0 there, so Jvar is the prior and dvar is 0, and the k* column is the bit-for-bit case of part A"""
    dtype = np_dtype(f32)
    sites = vx.pow2_sites(d)
    assert sites.size >= 4
    qsite = np.r_[sites[:70], vx.ORIGIN, sites[:3]]
    prior = dtype(vx.C) * dtype(vx.G0[kt])
    want = d.expected(dtype)[qsite]
    for flags in (dict(Jvar=True), dict(var=True, Jvar=True), dict(J=True, Jvar=True, dvar=True)):
        out = predict(h, d.queries(qsite), flags)
        assert np.all(out["Jvar"] == prior), flags
        if "var" in out:
            assert np.array_equal(out["var"], want), vx.describe_wrong(d, qsite, out["var"], want)
        if "dvar" in out:
            assert np.all(out["dvar"] == 0), flags


COLUMN_CASES = [(f32, kt, D, 1300) for f32 in (False, True) for kt in (0, 2, 3) for D in (2, 3, 4, 6, 8, 12)]
COLUMN_CASES += [(False, 0, 3, 512), (True, 2, 8, 512)]                 # every launch kind once at one i-block


@pytest.mark.parametrize("f32,kt,D,N", COLUMN_CASES, ids=lambda x: str(x))
def test_derivative_columns_calibrated(f32, kt, D, N, monkeypatch):
    monkeypatch.delenv("GPT_VAR_DIAG_HALF", raising=False)
    d = column_design(N, D, f32)
    h = column_model(d, kt, f32)
    worst = run_column_cases(h, [d], [1.0], kt, f32, vx.REQUESTS, single, monkeypatch, vx.NOISE)
    on_site_equalities(h, d, kt, f32)                        # (the design's own factor is still in place)
    h.close()
    for name, (r_op, r_pr) in worst.items():
        print(f"COLUMNS {'fp32' if f32 else 'fp64'} {KIND_NAMES[kt]} D={D} N={N} [{name}]: operand error / bound {r_op:.3f}, product error / bound {r_pr:.3f}")


@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_multitask_derivative_columns_calibrated(f32, D, monkeypatch):
    monkeypatch.delenv("GPT_VAR_DIAG_HALF", raising=False)
    N = 1300
    ds = [column_design(N, D, f32, task_seed(t, N), TASK_C[t]) for t in range(3)]
    h = svgp_model(ds, f32)
    worst = run_column_cases(h, ds, TASK_C, 0, f32, (dict(Jvar=True), dict(var=True, Jvar=True)), inject_tasks, monkeypatch, 0.0)
    h.close()
    for name, (r_op, r_pr) in worst.items():
        print(f"COLUMNS {'fp32' if f32 else 'fp64'} multi-task D={D} N={N} [{name}]: operand error / bound {r_op:.3f}, product error / bound {r_pr:.3f}")
