"""A batch of independent small exact GPs, one workgroup per model (csrc/gpt_batch.hip, GaussianProcessBatch,
GaussianProcessTransportationBatch): the reference's goldens through mixed batches, scikit-learn for the Matern kernels, the
oracle at every size where the factor takes another path, and the two bitwise invariants (a model does not depend on the
batch around it, a query not on the other queries)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT, assert_parity, load_golden

gpu = pytest.mark.gpu
RTOL = 1e-5           # north star, against goldens and the oracle
LML_TOL = 1e-6        # LML (relative) and gradients, as test_lml_value_and_gradient_vs_sklearn
NEW = ("gpt_batch_lml_objective", "gpt_batch_fit", "gpt_batch_predict")
OUTPUTS = ("mean", "var", "J", "Jvar", "dvar")


def sk_kernel(c, ls, noise, nu=None):
    from sklearn.gaussian_process.kernels import RBF, Matern, WhiteKernel, ConstantKernel as Ck
    ls = np.asarray(ls, dtype=float).tolist() if np.size(ls) > 1 else [float(np.ravel(ls)[0])]
    return Ck(float(c)) * (RBF(length_scale=ls) if nu is None else Matern(length_scale=ls, nu=nu)) + WhiteKernel(float(noise))


def problem(n, D=3, O=3, seed=0):
    """Seeded uniform data in the style of orc.synthetic_problem."""
    rng = np.random.default_rng(1000 * seed + n)
    X = rng.uniform(0, 1, (n, D))
    Y = 0.05 * np.sin(4 * X[:, np.arange(O) % D] + np.arange(O)) + 0.01 * rng.standard_normal((n, O))
    return X, Y


def oracle_posterior(xq, X, Y, c, ls, noise, jitter=1e-10):
    from oracle import gp_oracle as orc
    L, a = orc.gpr_fit(X, Y, c, ls, noise, jitter)
    mean, var, J, Jvar = orc.posterior_all_fast(xq, X, L, a, c, ls, noise, want_jvar=True)
    o = orc.GaussianProcessOracle(c, np.broadcast_to(ls, (X.shape[1],)), noise, jitter).fit(X, Y)
    return {"L": L, "alpha": a, "mean": mean, "var": var, "J": J, "Jvar": Jvar, "dvar": o.derivative_of_variance(xq).T}


# ------------------------------------------------------------------------------------------------------- CPU
def test_signature_table_and_header():
    from gaussian_process_transportation_amd import _lib
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [16, 17, 21]
    assert all(_lib.SIGNATURES[n][0] is C.c_int for n in NEW)
    header = open(os.path.join(ROOT, "include", "gpt_hip.h")).read()
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", header, flags=re.S)
        assert m and "model_gpt.py:74-83" in m.group(1), name
    stub = open(os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc", "host_stub", "stub_launchers.cpp")).read()
    for name in NEW:
        assert re.search(r'extern "C" int ' + name + r"\(", stub), name
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW)


def test_class_refusals_without_a_device():
    from gaussian_process_transportation_amd import GaussianProcessBatch, GaussianProcessTransportationBatch
    k = sk_kernel(1.0, [0.3], 1e-3)
    gp = GaussianProcessBatch(k, optimizer=None)
    X, Y = problem(10)
    with pytest.raises(ValueError, match="GaussianProcess"):
        gp.fit([X, np.zeros((129, 3))], [Y, np.zeros((129, 3))])
    Ynan = np.zeros((130, 3))
    Ynan[:2] = np.nan                                            # 128 rows after the filter: not refused for its size
    with pytest.raises(ValueError, match="D = 1 .. 15"):
        gp.fit([np.zeros((130, 16))], [Ynan])
    with pytest.raises(ValueError, match="share D and O"):
        gp.fit([X, np.zeros((5, 2))], [Y, np.zeros((5, 3))])
    with pytest.raises(ValueError, match="share D and O"):
        gp.fit([X, X], [Y, Y[:, :2]])
    with pytest.raises(ValueError, match="O = 1 .. 16"):
        gp.fit([X], [np.zeros((10, 17))])
    with pytest.raises(ValueError, match="different numbers of rows"):
        gp.fit([X], [Y[:5]])
    with pytest.raises(ValueError, match="length_scale has 2 entries"):
        GaussianProcessBatch(sk_kernel(1.0, [0.3, 0.3], 1e-3)).fit([X], [Y])        # before the search: no device needed
    with pytest.raises(ValueError, match="callable optimizer"):
        GaussianProcessBatch(k, optimizer=lambda f, x0, bounds: (x0, 0.0))
    with pytest.raises(ValueError, match="callable optimizer"):
        GaussianProcessTransportationBatch(k, optimizer=lambda f, x0, bounds: (x0, 0.0))
    with pytest.raises(RuntimeError, match="not fitted"):
        gp.predict([X])
    tr = GaussianProcessTransportationBatch(k, optimizer=None)
    with pytest.raises(AttributeError, match="source_distributions"):
        tr.fit_transportations()


def test_batch_pack_layout():
    from gaussian_process_transportation_amd import _lib
    Xs, Ys = zip(*(problem(n) for n in (3, 1, 7)))
    X, Y, nb = _lib.batch_pack(Xs, Ys)
    assert nb.dtype == np.int64 and nb.tolist() == [0, 3, 4, 11]
    assert X.flags.c_contiguous and np.array_equal(X[4:], Xs[2]) and np.array_equal(Y[3:4], Ys[1])


# ------------------------------------------------------------------------------------------------------- GPU: anchors
def _anchor_group(name):
    """(members [(X, Y)], golden, hyper-parameters): the fixture, a copy with permuted rows and a shorter copy."""
    g = load_golden(name)
    X, Y = (g["gp_X"], g["gp_Y"]) if name == "letterS_2d" else (g["X"], g["Y"])
    perm = np.random.default_rng(4).permutation(len(X))
    short = len(X) // 2 + 1
    return [(X, Y), (X[perm], Y[perm]), (X[:short], Y[:short])], g, perm


# what each fixture holds beyond L_ / alpha_ (letter-S: its predictions are the transport test's; the NaN fixture has no LML grid):
# a renamed key must fail the test, not skip its checks
ANCHOR_KEYS = {"letterS_2d": {"lml_fit"}, "synthetic_3d_N64": {"Xq", "lml_theta"}, "synthetic_3d_N64_iso": {"Xq", "lml_theta"},
               "synthetic_3d_N64_nan": {"Xq"}, "synthetic_15d_N96": {"Xq", "lml_theta"}, "synthetic_8d_N128": {"Xq", "lml_theta"}}


@gpu
@pytest.mark.parametrize("name", sorted(ANCHOR_KEYS))
def test_reference_anchor_in_a_ragged_batch(name):
    from gaussian_process_transportation_amd import GaussianProcessBatch, _lib
    members, g, perm = _anchor_group(name)
    assert {k for k in ("Xq", "lml_theta", "lml_fit") if k in g} == ANCHOR_KEYS[name], sorted(g)
    if "Xq" in g:
        assert {"mean", "mean_only", "std", "J", "Jvar", "dvar"} <= set(g)
    if "lml_theta" in g:
        assert {"lml_value", "lml_grad"} <= set(g)
    c, ls, noise, jitter = float(g["constant_value"]), g["length_scale"], float(g["noise_level"]), float(g["alpha"])
    if name == "synthetic_3d_N64_nan":                       # the three 3-D ARD problems share their hyper-parameters: one batch
        g64 = load_golden("synthetic_3d_N64")
        members[2] = (g64["X"], g64["Y"])
    gp = GaussianProcessBatch(sk_kernel(c, ls, noise), alpha=jitter, optimizer=None).fit(*zip(*members))
    keep = ~np.isnan(members[0][1]).any(axis=1)
    assert gp.Xs[0].shape[0] == g["alpha_"].shape[0] and len({len(x) for x in gp.Xs}) >= 2      # NaN rows dropped; ragged
    assert_parity(gp.L_[0], g["L_"], RTOL, "L_")
    assert np.all(np.triu(gp.L_[0], 1) == 0.0)
    assert_parity(gp.alpha_[0], g["alpha_"], RTOL, "alpha_")
    kept_perm = perm[keep[perm]]                             # the permuted copy after ITS filter, in fixture row numbers
    rank = np.cumsum(keep) - 1
    assert_parity(gp.alpha_[1], g["alpha_"][rank[kept_perm]], RTOL, "alpha_ of the permuted copy")
    if name == "synthetic_3d_N64_nan":
        assert_parity(gp.L_[2], g64["L_"], RTOL, "L_ of the N64 member")
    if "lml_fit" in g:
        assert gp.log_marginal_likelihood_values_[0] == pytest.approx(float(g["lml_fit"]), rel=LML_TOL)
    if "Xq" in g:
        Xq = g["Xq"]
        xs = [Xq, Xq, Xq[:7]]
        pred, der, dvar = gp.predict(xs, return_std=True), gp.derivative(xs, return_var=True), gp.derivative_of_variance(xs)
        mean_only, post = gp.predict(xs), gp.posterior(xs, jacobian_variance=True)
        for b in (0, 1):                                     # the same function, whatever the order of the rows
            assert_parity(pred[b][0], g["mean"], RTOL, f"mean [{b}]")
            assert_parity(pred[b][1], g["std"], RTOL, f"std [{b}]")
            assert_parity(mean_only[b], g["mean_only"], RTOL, f"mean only [{b}]")
            assert_parity(der[b][0], g["J"], RTOL, f"J [{b}]")
            assert_parity(der[b][1], g["Jvar"], RTOL, f"Jvar [{b}]")
            assert_parity(dvar[b], g["dvar"], RTOL, f"dvar [{b}]")
            assert_parity(np.sqrt(post[b]["var"]) - np.sqrt(noise), g["std"][:, 0], RTOL, f"fused std [{b}]")
            assert_parity(post[b]["Jvar"], g["Jvar"][:, 0, :], RTOL, f"fused Jvar [{b}]")
        assert pred[2][0].shape == (7, Xq.shape[1]) and dvar[2].shape == (Xq.shape[1], 7)
    if "lml_theta" in g:                                     # the fixture's three thetas as three models of one call
        n_ls = ls.size
        th = g["lml_theta"]
        X, Y = members[0]
        lml, grad, status = _lib.batch_lml_objective([X] * 3, [Y] * 3, np.exp(th[:, 1:1 + n_ls]), np.exp(th[:, 0]), np.exp(th[:, 1 + n_ls]),
                                                     jitter)
        assert status.tolist() == [0, 0, 0]
        for k in range(3):
            assert lml[k] == pytest.approx(float(g["lml_value"][k]), rel=LML_TOL)
            assert_parity(grad[k], g["lml_grad"][k], LML_TOL, f"d lml / d theta [{k}]")


@gpu
@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5])
def test_matern_objective_and_prediction_vs_sklearn(nu):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from gaussian_process_transportation_amd import GaussianProcessBatch, _lib
    members = [problem(17, 2, 2, seed=3), problem(65, 2, 2, seed=3), problem(9, 2, 2, seed=3)]
    c, ls, noise = 0.4, np.array([0.35, 0.6]), 2e-3
    kernel = sk_kernel(c, ls, noise, nu=nu)
    xq = np.random.default_rng(8).uniform(0, 1, (70, 2))
    gp = GaussianProcessBatch(kernel, optimizer=None).fit(*zip(*members))
    pred = gp.predict([xq] * 3, return_std=True)
    thetas = kernel.theta + np.array([[0.0] * 4, [0.3, -0.2, 0.1, 0.5], [-0.4, 0.2, 0.3, -1.0]])
    code = {0.5: 1, 1.5: 2, 2.5: 3}[nu]
    for b, (X, Y) in enumerate(members):
        ref = GaussianProcessRegressor(kernel=kernel, alpha=1e-10, optimizer=None).fit(X, Y)
        m, s = ref.predict(xq, return_std=True)
        assert_parity(pred[b][0], m, RTOL, f"mean, n = {len(X)}")
        assert_parity(pred[b][1] + np.sqrt(noise), s, RTOL, f"std, n = {len(X)}")
        lml, grad, status = _lib.batch_lml_objective([X] * 3, [Y] * 3, np.exp(thetas[:, 1:3]), np.exp(thetas[:, 0]), np.exp(thetas[:, 3]),
                                                     1e-10, kernel_type=code)
        for k in range(3):
            v, gr = ref.log_marginal_likelihood(thetas[k], eval_gradient=True)
            assert lml[k] == pytest.approx(v, rel=LML_TOL)
            assert_parity(grad[k], gr, LML_TOL, f"gradient, n = {len(X)}, theta {k}")
    with pytest.raises(NotImplementedError, match="RBF only"):
        gp.derivative([xq] * 3)


# ------------------------------------------------------------------------------------------------------- GPU: sizes
EDGE_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)


def _edge_batch():
    rng = np.random.default_rng(21)
    B = len(EDGE_SIZES)
    Xs, Ys = zip(*(problem(n) for n in EDGE_SIZES))
    return list(Xs), list(Ys), rng.uniform(0.15, 0.4, (B, 3)), rng.uniform(0.05, 0.2, B), rng.uniform(1e-4, 1e-3, B)


@gpu
def test_sizes_where_the_factor_can_go_wrong():
    """Both LDS instantiations (n <= 32, n <= 128) and their edges in one batch, against the oracle."""
    from gaussian_process_transportation_amd import _lib
    from oracle import gp_oracle as orc
    Xs, Ys, ls, c, noise = _edge_batch()
    xqs = [np.random.default_rng(30 + b).uniform(0, 1, (11, 3)) for b in range(len(Xs))]
    Ls, alphas, lml_fit, status = _lib.batch_fit(Xs, Ys, ls, c, noise, 1e-10)
    out, status_p = _lib.batch_predict(Xs, Ys, ls, c, noise, 1e-10, xqs, mean=True, var=True, J=True, Jvar=True, dvar=True)
    lml, grad, status_o = _lib.batch_lml_objective(Xs, Ys, ls, c, noise, 1e-10)
    assert not status.any() and not status_p.any() and not status_o.any()
    for b, n in enumerate(EDGE_SIZES):
        ref = oracle_posterior(xqs[b], Xs[b], Ys[b], c[b], ls[b], noise[b])
        assert_parity(Ls[b], ref["L"], RTOL, f"L, n = {n}")
        assert np.all(np.triu(Ls[b], 1) == 0.0)
        assert_parity(alphas[b], ref["alpha"], RTOL, f"alpha, n = {n}")
        for k in OUTPUTS:
            assert_parity(out[k][b], ref[k], RTOL, f"{k}, n = {n}")
        v, g = orc.log_marginal_likelihood(np.log(np.concatenate([[c[b]], ls[b], [noise[b]]])), Xs[b], Ys[b], 3, alpha=1e-10)
        assert lml[b] == pytest.approx(v, rel=LML_TOL) and lml_fit[b] == pytest.approx(v, rel=LML_TOL)
        assert_parity(grad[b], g, LML_TOL, f"gradient, n = {n}")


@gpu
def test_grid_wrap_more_models_than_compute_units():
    from gaussian_process_transportation_amd import _lib
    from oracle import gp_oracle as orc
    B = 600
    rng = np.random.default_rng(5)
    Xs, Ys = zip(*(problem(5, 2, 2, seed=100 + b) for b in range(B)))
    ls, c, noise = rng.uniform(0.2, 0.5, (B, 2)), rng.uniform(0.5, 1.5, B), rng.uniform(1e-3, 1e-2, B)
    xqs = [rng.uniform(0, 1, (3, 2)) for _ in range(B)]
    Ls, alphas, _, status = _lib.batch_fit(Xs, Ys, ls, c, noise, 1e-10)
    out, _ = _lib.batch_predict(Xs, Ys, ls, c, noise, 1e-10, xqs, mean=True, var=True, J=True, Jvar=True, dvar=True)
    lml, grad, _ = _lib.batch_lml_objective(Xs, Ys, ls, c, noise, 1e-10)
    assert not status.any()
    for b in [0, 599] + sorted(np.random.default_rng(6).choice(np.arange(1, 599), 3, replace=False).tolist()):
        ref = oracle_posterior(xqs[b], Xs[b], Ys[b], c[b], ls[b], noise[b])
        assert_parity(Ls[b], ref["L"], RTOL, f"L [{b}]")
        assert_parity(alphas[b], ref["alpha"], RTOL, f"alpha [{b}]")
        for k in OUTPUTS:
            assert_parity(out[k][b], ref[k], RTOL, f"{k} [{b}]")
        v, g = orc.log_marginal_likelihood(np.log(np.concatenate([[c[b]], ls[b], [noise[b]]])), Xs[b], Ys[b], 2, alpha=1e-10)
        assert lml[b] == pytest.approx(v, rel=LML_TOL)
        assert_parity(grad[b], g, LML_TOL, f"gradient [{b}]")


@gpu
def test_query_tiles_and_query_independence():
    from gaussian_process_transportation_amd import _lib
    counts = (0, 1, 63, 64, 65, 257)
    Xs, Ys = zip(*(problem(n) for n in (12, 40, 7, 33, 20, 50)))
    rng = np.random.default_rng(9)
    ls, c, noise = rng.uniform(0.15, 0.4, (6, 3)), rng.uniform(0.05, 0.2, 6), rng.uniform(1e-4, 1e-3, 6)
    xqs = [rng.uniform(0, 1, (m, 3)) for m in counts]
    want = dict(mean=True, var=True, J=True, Jvar=True, dvar=True)
    out, status = _lib.batch_predict(Xs, Ys, ls, c, noise, 1e-10, xqs, **want)
    assert not status.any()
    for b, m in enumerate(counts):
        assert out["mean"][b].shape == (m, 3) and out["J"][b].shape == (m, 3, 3) and out["dvar"][b].shape == (m, 3)
        if m:
            ref = oracle_posterior(xqs[b], Xs[b], Ys[b], c[b], ls[b], noise[b])
            for k in OUTPUTS:
                assert_parity(out[k][b], ref[k], RTOL, f"{k}, M = {m}")
    # a query's results do not depend on the other queries: rows [10, 40) of a member, alone
    for b in (5, 2):
        part, _ = _lib.batch_predict([Xs[b]], [Ys[b]], ls[b:b + 1], c[b:b + 1], noise[b:b + 1], 1e-10, [xqs[b][10:40]], **want)
        for k in OUTPUTS:
            assert np.array_equal(part[k][0], out[k][b][10:40]), (k, b)


@gpu
def test_a_model_does_not_depend_on_the_batch_around_it():
    from gaussian_process_transportation_amd import _lib
    sizes = (9, 70, 30, 128, 33, 5, 64)
    Xs, Ys = map(list, zip(*(problem(n, seed=2) for n in sizes)))
    rng = np.random.default_rng(12)
    B = len(sizes)
    ls, c, noise = rng.uniform(0.15, 0.4, (B, 3)), rng.uniform(0.05, 0.2, B), rng.uniform(1e-4, 1e-3, B)
    xqs = [rng.uniform(0, 1, (20 + 9 * b, 3)) for b in range(B)]
    want = dict(mean=True, var=True, J=True, Jvar=True, dvar=True)

    def run(order):
        o = list(order)
        args = ([Xs[b] for b in o], [Ys[b] for b in o], ls[o], c[o], noise[o], 1e-10)
        L, a, lml_f, _ = _lib.batch_fit(*args)
        lml, grad, _ = _lib.batch_lml_objective(*args)
        out, _ = _lib.batch_predict(*args, [xqs[b] for b in o], **want)
        return {b: dict(L=L[k], alpha=a[k], lml_fit=lml_f[k], lml=lml[k], grad=grad[k], **{n: out[n][k] for n in OUTPUTS})
                for k, b in enumerate(o)}

    for target in (2, 4):                          # one model of each size class (n = 30, n = 33)
        others = [b for b in range(B) if b != target]
        alone = run([target])[target]
        for order in ([target] + others, others + [target], others[:3] + [target] + others[3:]):
            got = run(order)[target]
            for k, v in alone.items():
                assert np.array_equal(got[k], v), (k, target, order)


# ------------------------------------------------------------------------------------------------------- GPU: raw ABI
def _ptr(a, ty=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(ty))


def _raw(entry, Xs, Ys, ls0, c0, noise0, jitter, ktype, tail, **override):
    """One call through the C ABI on arrays the test owns (pre-filled outputs stay observable).  override: any leading
    argument by name, to break one limit at a time."""
    from gaussian_process_transportation_amd import _lib
    lib = _lib.load()
    X, Y = np.ascontiguousarray(np.concatenate(Xs)), np.ascontiguousarray(np.concatenate(Ys))
    nb = np.concatenate([[0], np.cumsum([len(x) for x in Xs])]).astype(np.int64)
    a = dict(X=X, Y=Y, n_begin=nb, B=len(Xs), D=X.shape[1], O=Y.shape[1], ls=np.ascontiguousarray(ls0, dtype=np.float64),
             n_ls=np.shape(ls0)[1], c=np.ascontiguousarray(c0, dtype=np.float64), noise=np.ascontiguousarray(noise0, dtype=np.float64))
    a.update(override)
    rc = getattr(lib, entry)(0, _ptr(a["X"]), _ptr(a["Y"]), _ptr(a["n_begin"], C.c_int64), a["B"], a["D"], a["O"], _ptr(a["ls"]), a["n_ls"],
                             _ptr(a["c"]), _ptr(a["noise"]), float(jitter), int(ktype), *tail)
    return rc, _lib.last_error()


def _not_pd_models():
    Xs, Ys = map(list, zip(*(problem(n, 2, 2, seed=7) for n in (12, 6, 40))))
    Xs[1][1] = Xs[1][0]                            # rows 0 and 1 identical; c = 1, noise 0, jitter 0: second pivot 1 - 1 * 1 = 0
    ls = np.array([[0.3, 0.4], [0.5, 0.5], [0.25, 0.3]])
    return Xs, Ys, ls, np.array([0.7, 1.0, 1.3]), np.array([1e-3, 0.0, 2e-3])


@gpu
def test_not_pd_model_is_isolated():
    from gaussian_process_transportation_amd import GaussianProcessBatch, _lib
    Xs, Ys, ls, c, noise = _not_pd_models()
    xqs = [np.random.default_rng(b).uniform(0, 1, (m, 2)) for b, m in enumerate((5, 70, 9))]
    Xq = np.concatenate(xqs)
    qb = np.array([0, 5, 75, 84], dtype=np.int64)
    FILL = 7.25

    def call(models):
        n = [len(Xs[b]) for b in models]
        M = sum(len(xqs[b]) for b in models)
        o = dict(L=np.full(sum(k * k for k in n), FILL), alpha=np.full((sum(n), 2), FILL), lml_fit=np.full(len(n), FILL),
                 lml=np.full(len(n), FILL), grad=np.full((len(n), 4), FILL), mean=np.full((M, 2), FILL), var=np.full(M, FILL),
                 J=np.full((M, 2, 2), FILL), Jvar=np.full((M, 2), FILL), dvar=np.full((M, 2), FILL))
        st = [np.full(len(n), 99, dtype=np.int32) for _ in range(3)]
        args = ([Xs[b] for b in models], [Ys[b] for b in models], ls[models], c[models], noise[models], 0.0, 0)
        q = np.concatenate([[0], np.cumsum([len(xqs[b]) for b in models])]).astype(np.int64)
        xq = np.ascontiguousarray(np.concatenate([xqs[b] for b in models]))
        assert _raw("gpt_batch_fit", *args, (_ptr(o["L"]), _ptr(o["alpha"]), _ptr(o["lml_fit"]), _ptr(st[0], C.c_int)))[0] == 0
        assert _raw("gpt_batch_lml_objective", *args, (_ptr(o["lml"]), _ptr(o["grad"]), _ptr(st[1], C.c_int)))[0] == 0
        assert _raw("gpt_batch_predict", *args, (_ptr(xq), _ptr(q, C.c_int64), _ptr(o["mean"]), _ptr(o["var"]), _ptr(o["J"]), _ptr(o["Jvar"]),
                                                 _ptr(o["dvar"]), _ptr(st[2], C.c_int)))[0] == 0
        return o, st, np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum([k * k for k in n])]), q

    o, st, nb, lb, q = call([0, 1, 2])
    for s in st:
        assert s.tolist() == [0, _lib.GPT_E_NOT_PD, 0]
    assert np.all(o["L"][lb[1]:lb[2]] == FILL) and np.all(o["alpha"][nb[1]:nb[2]] == FILL)
    assert o["lml_fit"][1] == FILL and o["lml"][1] == FILL and np.all(o["grad"][1] == FILL)
    for k in OUTPUTS:
        assert np.all(o[k][q[1]:q[2]] == FILL), k
    o2, st2, nb2, lb2, q2 = call([0, 2])
    assert all(s.tolist() == [0, 0] for s in st2)
    for src, dst in ((0, 0), (2, 1)):                        # models 0 and 2: bit for bit the batch without model 1
        assert np.array_equal(o["L"][lb[src]:lb[src + 1]], o2["L"][lb2[dst]:lb2[dst + 1]])
        assert np.array_equal(o["alpha"][nb[src]:nb[src + 1]], o2["alpha"][nb2[dst]:nb2[dst + 1]])
        for k in ("lml_fit", "lml", "grad"):
            assert np.array_equal(o[k][src], o2[k][dst]), k
        for k in OUTPUTS:
            assert np.array_equal(o[k][q[src]:q[src + 1]], o2[k][q2[dst]:q2[dst + 1]]), k
        assert not np.any(o["mean"][q[src]:q[src + 1]] == FILL)
    # the class: same kernel for every member, so the degenerate member fails at c = 1, noise 0, alpha 0 and the others do not
    gp = GaussianProcessBatch(sk_kernel(1.0, [0.2, 0.2], 0.0), alpha=0.0, optimizer=None)
    with pytest.raises(np.linalg.LinAlgError, match=r"model\(s\) \[1\]"):
        gp.fit([Xs[0][:6], Xs[1], Xs[2][:6]], [Ys[0][:6], Ys[1], Ys[2][:6]])


@gpu
def test_refusals_through_the_c_abi():
    from gaussian_process_transportation_amd import _lib
    Xs, Ys = map(list, zip(*(problem(n, 2, 2, seed=7) for n in (12, 6, 40))))
    ls, c, noise = np.full((3, 2), 0.3), np.ones(3), np.full(3, 1e-3)
    lml, grad, st = np.zeros(3), np.zeros((3, 4)), np.zeros(3, dtype=np.int32)
    tail = (_ptr(lml), _ptr(grad), _ptr(st, C.c_int))

    def refused(match, entry="gpt_batch_lml_objective", tail=tail, jitter=1e-10, ktype=0, **override):
        rc, msg = _raw(entry, Xs, Ys, ls, c, noise, jitter, ktype, tail, **override)
        assert rc == _lib.GPT_E_ARG and re.search(match, msg), (rc, msg, override)

    assert _raw("gpt_batch_lml_objective", Xs, Ys, ls, c, noise, 1e-10, 0, tail)[0] == 0
    big = np.zeros((200, 2))
    refused("n_b <= 128", X=big, Y=big, n_begin=np.array([0, 129, 135, 175], dtype=np.int64))
    refused("n_b <= 128", n_begin=np.array([0, 12, 12, 58], dtype=np.int64))              # an empty model
    refused("n_b <= 128", n_begin=np.array([0, 18, 12, 58], dtype=np.int64))              # offsets that go back
    refused(r"n_begin\[0\]", n_begin=np.array([1, 12, 18, 58], dtype=np.int64))
    refused("D must be 1 .. 15", D=16)
    refused("D must be 1 .. 15", D=0)
    refused("O .* 1 .. 16", O=17)
    refused("O .* 1 .. 16", O=0)
    refused(r"1 .. 2\^20", B=0)
    refused(r"1 .. 2\^20", B=(1 << 20) + 1)
    refused("n_ls must be 1 or D", n_ls=3)
    refused("kernel_type", ktype=4)
    refused("alpha_jitter", jitter=-1.0)
    refused("alpha_jitter", jitter=np.nan)
    for bad in (np.nan, np.inf):
        Xb = np.concatenate(Xs)
        Xb[20, 1] = bad
        refused("NaN or infinity", X=Xb)
        Yb = np.concatenate(Ys)
        Yb[57, 0] = bad
        refused("NaN or infinity", Y=Yb)
        refused("length_scale", ls=np.array([[0.3, 0.3], [0.3, bad], [0.3, 0.3]]))
        refused("constant_value", c=np.array([1.0, bad, 1.0]))
        refused("constant_value", noise=np.array([1e-3, 1e-3, bad]))
    refused("length_scale", ls=np.array([[0.3, 0.3], [0.3, 0.0], [0.3, 0.3]]))
    refused("constant_value", c=np.array([1.0, 0.0, 1.0]))
    refused("noise_level >= 0", noise=np.array([1e-3, -1e-9, 1e-3]))
    refused("NULL", X=None)
    # the queries of gpt_batch_predict
    xq = np.random.default_rng(1).uniform(0, 1, (30, 2))
    mean, J = np.zeros((30, 2)), np.zeros((30, 2, 2))

    def ptail(q, xq=xq, mean=mean, J=None):
        return (_ptr(xq), _ptr(np.asarray(q, dtype=np.int64), C.c_int64), _ptr(mean), None, _ptr(J), None, None, _ptr(st, C.c_int))

    assert _raw("gpt_batch_predict", Xs, Ys, ls, c, noise, 1e-10, 0, ptail([0, 10, 10, 30]))[0] == 0        # M_b = 0 is fine
    refused("q_begin must not decrease", "gpt_batch_predict", ptail([0, 10, 5, 30]))
    refused(r"q_begin\[0\]", "gpt_batch_predict", ptail([2, 10, 20, 30]))
    refused(r"fewer than 2\^31", "gpt_batch_predict", ptail([0, 10, 20, 1 << 31]))
    xbad = xq.copy()
    xbad[3, 0] = np.nan
    refused("Xq contains NaN", "gpt_batch_predict", ptail([0, 10, 20, 30], xq=xbad))
    for ktype in (1, 2, 3):                                  # derivative outputs on a Matern batch
        refused("RBF only", "gpt_batch_predict", ptail([0, 10, 20, 30], J=J), ktype=ktype)
        assert _raw("gpt_batch_predict", Xs, Ys, ls, c, noise, 1e-10, ktype, ptail([0, 10, 20, 30]))[0] == 0


# ------------------------------------------------------------------------------------------------------- GPU: optimiser, transport
@gpu
def test_letterS_optimizer_inside_a_batch():
    """The letter-S problem as model 2 of four under np.random.seed(0): theta and LML as the reference's own fit, to the bounds
    test_letterS_with_optimizer_matches_reference_fit holds the single-model path to."""
    from gaussian_process_transportation_amd import GaussianProcessBatch
    g = load_golden("letterS_2d")
    others = [problem(10, 2, 2, seed=40 + k) for k in range(3)]
    members = others[:2] + [(g["gp_X"], g["gp_Y"])] + others[2:]
    np.random.seed(0)
    gp = GaussianProcessBatch(sk_kernel(10.0, 4 * np.ones(2), 0.01)).fit(*zip(*members))
    lml_ref = float(g["lml_fit"])
    print("letter-S in a batch: theta", gp.kernels_[2].theta, "reference", g["theta_fit"], "lml", gp.log_marginal_likelihood_values_[2],
          lml_ref, "batched objective calls", gp.optimizer_stats_["calls"])
    assert gp.log_marginal_likelihood_values_[2] == pytest.approx(lml_ref, rel=1e-6)
    assert_parity(np.asarray(gp.kernels_[2].theta), g["theta_fit"], 1e-6, "fitted theta")
    assert len(gp.kernels_) == 4 and all(np.isfinite(gp.log_marginal_likelihood_values_))


@gpu
def test_transport_batch_against_the_golden_and_the_single_model_class():
    from gaussian_process_transportation_amd import GaussianProcessTransportation, GaussianProcessTransportationBatch
    g = load_golden("letterS_2d")
    kernel = sk_kernel(g["constant_value"], g["length_scale"], g["noise_level"])
    rng = np.random.default_rng(17)
    pairs = []
    for n, m in ((10, 200), (15, 90)):
        src = rng.uniform(-20, 20, (n, 2))
        ang = rng.uniform(0, 1)
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        tgt = src @ R.T + rng.uniform(-5, 5, 2) + 0.8 * np.sin(src / 7.0)
        traj = np.column_stack([np.linspace(-18, 18, m), 10 * np.sin(np.linspace(0, 3, m))])
        pairs.append((src, tgt, traj, np.gradient(traj, axis=0)))
    pairs.insert(1, (g["source"], g["target"], g["demo"], g["delta"]))
    tb = GaussianProcessTransportationBatch(kernel_transport=kernel, optimizer=None)
    tb.source_distributions, tb.target_distributions, tb.training_trajs, tb.training_deltas = map(list, zip(*pairs))
    tb.fit_transportations(do_scale=False, do_rotation=True)
    tb.apply_transportations()
    for name, got in (("traj", tb.training_trajs[1]), ("std", tb.stds[1]), ("vel", tb.training_deltas[1]), ("var_vel", tb.var_vels_transported[1])):
        assert_parity(got, g[name], RTOL, name)
    assert tb.training_trajs_old[1] is g["demo"]
    for b, (src, tgt, traj, vel) in enumerate(pairs):
        tr = GaussianProcessTransportation(kernel_transport=kernel, optimizer=None, verbose=False)
        tr.source_distribution, tr.target_distribution, tr.training_traj, tr.training_delta = src, tgt, traj, vel
        tr.fit_transportation(do_scale=False, do_rotation=True)
        tr.apply_transportation()
        for name, got, ref in (("traj", tb.training_trajs[b], tr.training_traj), ("std", tb.stds[b], tr.std),
                               ("vel", tb.training_deltas[b], tr.training_delta), ("var_vel", tb.var_vels_transported[b], tr.var_vel_transported)):
            scale = np.max(np.abs(ref))
            print(f"pair {b} {name}: batch vs single {np.max(np.abs(got - ref)) / scale:.2e}")
            assert_parity(got, ref, 1e-9, f"{name} of pair {b} vs GaussianProcessTransportation alone")
    # without velocities: positions and std only
    tb2 = GaussianProcessTransportationBatch(kernel_transport=kernel, optimizer=None)
    tb2.source_distributions, tb2.target_distributions, tb2.training_trajs = [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs]
    tb2.fit_transportations()
    tb2.apply_transportations()
    assert not hasattr(tb2, "var_vels_transported")
    for b in range(3):
        assert_parity(tb2.training_trajs[b], tb.training_trajs[b], 1e-12, "traj without velocities")
        assert_parity(tb2.stds[b], tb.stds[b], 1e-12, "std without velocities")
