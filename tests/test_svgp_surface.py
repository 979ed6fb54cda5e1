"""The point-cloud surface SVGP (svgp_surface.py; gpt_svgp_surface_train / _elbo_grad / _predict): the fp64 restatement
with a length-scale per task (tests/svgp_surface_restatement.py) on the CPU; on the GPU the device-wide step against
autograd, gpt_svgp_train (T = 1), torch.optim.Adam and the Titsias optimum, the predictive against the exact-GP goldens,
the reference's point clouds end to end, determinism and the not-positive-definite contract.
PARITY WITH GPYTORCH UNPINNED (not available): the restatement is this repository's reading of its defaults."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.linalg import cho_solve, solve_triangular

from tests import svgp_surface_restatement as ss
from tests.conftest import ROOT, load_golden, relmax

EPS = ss.JITTER
CLOUDS = ["distribution", "dustbin_cover", "pan", "white_towelholder", "wood_plate"]
NEW_SYMBOLS = ["gpt_svgp_surface_train", "gpt_svgp_surface_elbo_grad", "gpt_svgp_surface_predict"]


def _problem(Zn, T, D, N, seed=0, distinct=False):
    """Smooth multi-output data on [0,1]^D, inducing points drawn from it (distinct: without repeats), a random
    lower-triangular C, random m and distinct raw length-scales per task."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([0.3 * np.sin(3 * X @ rng.standard_normal(D) / np.sqrt(D) + t) for t in range(T)], 1)
    p = ss.init_params(X, Y, rng.choice(N, Zn, replace=not distinct))
    p["C"] = np.tril(0.05 * rng.standard_normal((T, Zn, Zn)), -1) + np.eye(Zn) * rng.uniform(0.5, 1.0, (T, 1, Zn))
    p["m"] = 0.1 * rng.standard_normal((T, Zn))
    p["raw_ls"] = rng.uniform(-1.5, -0.5, (T, D)) + np.log(D) / 2
    p["raw_os"] = rng.uniform(-1.0, 0.5, T)
    p["raw_noise"] = rng.uniform(-6.0, -3.0, T + 1)
    return X, Y, p


def _cloud(name):
    path = os.path.join(ROOT, "tests", "golden", f"point_cloud_{name}.npz")
    with np.load(path) as f:
        return np.asarray(f["cloud"], np.float64)


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_restatement_kl_matches_closed_form_with_distinct_lengthscales():
    """lik + KL / num_data: two num_data values isolate the KL, which must equal the numpy closed form; the per-task
    length-scales must actually enter (another task's l changes the loss of that task only)."""
    X, Y, p = _problem(12, 3, 2, 40, seed=3)
    assert np.ptp(p["raw_ls"], axis=0).min() > 0
    l1, g1 = ss.loss_and_grad(p, X[:10], Y[:10], 40)
    l2, _ = ss.loss_and_grad(p, X[:10], Y[:10], 400)
    kl = (l1 - l2) / (1 / 40 - 1 / 400)
    ref = sum(ss.kl_numpy(p["m"][t], p["C"][t]) for t in range(3))
    assert abs(kl - ref) <= 1e-9 * abs(ref)
    assert g1["raw_ls"].shape == (3, 2) and np.all(np.abs(g1["raw_ls"]) > 0)


def test_new_symbols_are_declared_bound_and_stubbed():
    from gaussian_process_transportation_amd import _lib
    with open(os.path.join(ROOT, "include", "gpt_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc", "host_stub", "stub_launchers.cpp")) as f:
        stub = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r'extern "C" int ' + name + r"\(", stub), name
    assert len(_lib.SIGNATURES["gpt_svgp_surface_train"][1]) == 19
    assert len(_lib.SIGNATURES["gpt_svgp_surface_elbo_grad"][1]) == 21
    assert len(_lib.SIGNATURES["gpt_svgp_surface_predict"][1]) == 14
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)


def test_surface_svgp_is_exported_next_to_the_transport_class():
    import gaussian_process_transportation_amd as pkg
    from gaussian_process_transportation_amd import svgp_exact, svgp_surface
    assert pkg.SurfaceSVGP is svgp_surface.StocasticVariationalGaussianProcess
    assert pkg.StocasticVariationalGaussianProcess is svgp_exact.StocasticVariationalGaussianProcess
    assert pkg.SurfaceSVGP.__name__ == "StocasticVariationalGaussianProcess"


def test_constructor_draws_inducing_points_like_the_reference():
    from gaussian_process_transportation_amd import SurfaceSVGP
    X = np.random.default_rng(0).uniform(0, 1, (50, 2))
    np.random.seed(4)
    model = SurfaceSVGP(X, X[:, :1], num_inducing=30)
    np.random.seed(4)
    expect = X[np.random.choice(np.arange(50), 30)]
    p = model.variational_params_
    assert np.array_equal(p["Z"], expect)
    assert not p["m"].any() and np.array_equal(p["C"], np.tile(np.eye(30), (1, 1, 1)))
    assert p["raw_ls"].shape == (1, 2) and not p["raw_ls"].any()


def test_argument_refusals_come_before_the_library(monkeypatch):
    """Bad shapes and limits raise ValueError naming the limit without loading the library (no GPU needed)."""
    from gaussian_process_transportation_amd import _lib, SurfaceSVGP

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    X, Y, p = _problem(10, 2, 2, 30)
    bb = np.array([0, 10])
    idx = np.arange(30)
    with pytest.raises(ValueError, match="4096"):
        SurfaceSVGP(np.zeros((5000, 2)), np.zeros((5000, 1)), num_inducing=4097)
    with pytest.raises(ValueError, match="32"):
        SurfaceSVGP(X, np.zeros((30, 33)), num_inducing=5)
    with pytest.raises(ValueError, match="1 .. 15"):
        SurfaceSVGP(np.zeros((30, 16)), Y, num_inducing=5)
    with pytest.raises(ValueError, match="1024"):
        SurfaceSVGP(X, Y, num_inducing=5).fit(num_epochs=1, batch_size=1025)
    with pytest.raises(ValueError, match="raw_ls"):
        _lib.svgp_surface_train(X, Y, dict(p, raw_ls=np.zeros(2)), idx, bb)
    with pytest.raises(ValueError, match="empty schedule"):
        _lib.svgp_surface_train(X, Y, p, idx, np.array([0]))
    with pytest.raises(ValueError, match=r"\[0, N\)"):
        _lib.svgp_surface_train(X, Y, p, np.full(30, 30), bb)
    with pytest.raises(ValueError, match="NaN"):
        _lib.svgp_surface_train(np.full((30, 2), np.nan), Y, p, idx, bb)
    with pytest.raises(ValueError, match="1 .. 1024"):
        _lib.svgp_surface_elbo_grad(np.zeros((1025, 2)), np.zeros((1025, 2)), p, 30)
    with pytest.raises(ValueError, match="columns"):
        _lib.svgp_surface_predict(p, np.zeros((4, 3)))


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("case", [(1000, 1, 2, 10), (37, 3, 3, 7), (300, 2, 15, 64)], ids=lambda c: "Z%d_T%d_D%d_b%d" % c)
def test_elbo_grad_matches_autograd(case):
    from gaussian_process_transportation_amd import _lib
    Zn, T, D, b = case
    X, Y, p = _problem(Zn, T, D, max(2 * b, 80), seed=Zn + D)
    lr, gr = ss.loss_and_grad(p, X[:b], Y[:b], len(X))
    lg, gg = _lib.svgp_surface_elbo_grad(X[:b], Y[:b], p, len(X))
    print(f"{case}: loss {abs(lg - lr) / abs(lr):.2e}", {k: f"{relmax(gg[k], gr[k]):.2e}" for k in ss.PARAM_NAMES})
    assert abs(lg - lr) <= 1e-10 * abs(lr)
    for k in ss.PARAM_NAMES:
        ref = np.tril(gr[k]) if k == "C" else gr[k]
        assert relmax(gg[k], ref) <= 1e-10, k


def _loss_explicit_inverse(tp, Xb, Yb, num_data):
    """ss.loss written the way the device computes it: W = L^-1 formed explicitly, A = W k(Z, X_b), U = C^T A,
    v = c + eps + |U_k|^2 - |A_k|^2, tr S = |C|_F^2 (torch fp64 on the CPU).  A second correct fp64 formulation: its
    disagreement with the restatement is the size of error that conditioning alone explains."""
    import torch
    import torch.nn.functional as F
    Z, m, C = tp["Z"], tp["m"], tp["C"]
    Zn, T, b = Z.shape[0], m.shape[0], Xb.shape[0]
    ls, c = F.softplus(tp["raw_ls"]), F.softplus(tp["raw_os"])
    noise = (ss.NOISE_FLOOR + F.softplus(tp["raw_noise"][:T])) + (ss.NOISE_FLOOR + F.softplus(tp["raw_noise"][T]))
    eye = torch.eye(Zn, dtype=Z.dtype)
    total = Z.new_zeros(())
    for t in range(T):
        L = torch.linalg.cholesky(c[t] * ss.rbf(Z, Z, ls[t]) + EPS * eye)
        W = torch.linalg.solve_triangular(L, eye, upper=False)
        A = W @ (c[t] * ss.rbf(Z, Xb, ls[t]))
        Ct = torch.tril(C[t])
        U = Ct.T @ A
        v = c[t] + EPS + (U * U).sum(0) - (A * A).sum(0)
        lik = -0.5 * torch.log(2 * np.pi * noise[t]) - ((Yb[:, t] - A.T @ m[t]) ** 2 + v) / (2 * noise[t])
        kl = 0.5 * ((Ct * Ct).sum() + m[t] @ m[t] - Zn - torch.log(torch.diagonal(Ct) ** 2).sum())
        total = total - lik.sum() / b + kl / num_data
    return total


def _loss_and_grad_explicit_inverse(p, Xb, Yb, num_data):
    import torch
    tp = ss.to_torch(p, requires_grad=True)
    val = _loss_explicit_inverse(tp, torch.as_tensor(np.asarray(Xb, np.float64)), torch.as_tensor(np.asarray(Yb, np.float64)), num_data)
    val.backward()
    return float(val.detach()), {k: tp[k].grad.numpy().copy() for k in ss.PARAM_NAMES}


# (Z, T, D, b): every boundary of the padded sizes NP = round_up(Z, 512) and BP = round_up(b, 64) and of the documented
# limits Z <= 4096, b <= 1024, T <= 32, D <= 15.  From NP = 2048 the NP x NP products run at tile edge 64 (256 tiles), among
# them the general A^T B ones (U = C^T A needs BP = 1024 as well: 16 x 8 x 2 tiles).
LIMIT_CASES = [(1, 2, 1, 1), (2, 32, 2, 63), (512, 1, 3, 65), (513, 2, 15, 1000), (1025, 1, 2, 1024), (1600, 2, 3, 200),
               (2200, 1, 3, 1024), (4096, 1, 2, 100), (64, 4, 15, 1024)]
FLOOR, SLACK, CAP = 1e-10, 10.0, 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("case", LIMIT_CASES, ids=lambda c: "Z%d_T%d_D%d_b%d" % c)
def test_elbo_grad_matches_autograd_at_the_size_limits(case):
    """Loss and gradients against the restatement where K(Z,Z) + 1e-4 I is no longer well conditioned.  The bound per
    quantity is max(1e-10, 10 d): d is the disagreement, on the CPU, of the explicit-inverse formulation with the restatement
    (two correct fp64 formulations of one objective); 10x because the device sums in another order again and inverts in
    blocks.  10 d <= 1e-8 is asserted, so conditioning never loosens a bound by more than two digits (inducing points are
    drawn without repeats to keep it so)."""
    from gaussian_process_transportation_amd import _lib
    Zn, T, D, b = case
    X, Y, p = _problem(Zn, T, D, max(2 * b, Zn + 50), seed=Zn + D, distinct=True)
    lr, gr = ss.loss_and_grad(p, X[:b], Y[:b], len(X))
    li, gi = _loss_and_grad_explicit_inverse(p, X[:b], Y[:b], len(X))
    lg, gg = _lib.svgp_surface_elbo_grad(X[:b], Y[:b], p, len(X))
    d = {"loss": abs(li - lr) / abs(lr), **{k: relmax(gi[k], gr[k]) for k in ss.PARAM_NAMES}}
    err = {"loss": abs(lg - lr) / abs(lr), **{k: relmax(gg[k], np.tril(gr[k]) if k == "C" else gr[k]) for k in ss.PARAM_NAMES}}
    print(f"{case}: " + ", ".join(f"{k} d {d[k]:.1e} gpu {err[k]:.1e}" for k in d))
    for k in d:
        assert SLACK * d[k] <= CAP, (k, d[k])
    for k in d:
        assert err[k] <= max(FLOOR, SLACK * d[k]), (k, err[k], d[k])


def _uneven_schedule():
    """T = 2, Z = 300; six batches, the largest first (every later step runs in a workspace wider than its batch), the
    schedule drawn with replacement (rows repeat inside a batch)."""
    X, Y, p = _problem(300, 2, 2, 1500, seed=11, distinct=True)
    sizes = [1024, 7, 64, 65, 1, 130]
    idx = np.random.default_rng(4).integers(0, 1500, sum(sizes))
    assert len(np.unique(idx[:1024])) < 1024 and len(np.unique(idx[1024:1031])) <= 7
    return X, Y, p, idx, np.concatenate([[0], np.cumsum(sizes)])


UNEVEN_LR = 1e-4


@pytest.mark.gpu
def test_uneven_batches_match_torch_adam(monkeypatch):
    """Six steps on batches of 1024, 7, 64, 65, 1 and 130 rows against torch.optim.Adam, to this file's 1e-9.
    Adam divides each gradient component by its own running magnitude, so a component near zero (d loss / d C_ij of two
    distant inducing points, 1e-9 against 13 for the largest) turns its rounding error, relative to ITSELF, into a step of
    lr times that: with inducing points drawn with repeats and lr = 0.01 two correct CPU formulations (the restatement and
    the explicit-inverse one) already end 7.8e-9 apart in C on this schedule, and with distinct points and lr = 1e-3 still
    0.65e-10 to 1.3e-10, depending on the machine's BLAS.  The inputs are therefore chosen (distinct inducing points,
    lr = 1e-4) so that those two agree to 1e-10, a tenth of the bound, with room to spare; that is asserted first.  What
    this test is for, a stale column of the wider workspace entering a gradient, is an error of the size of the gradient."""
    from gaussian_process_transportation_amd import _lib
    X, Y, p, idx, bb = _uneven_schedule()
    ref, tr_ref = ss.adam_train(p, X, Y, idx, bb, lr=UNEVEN_LR)
    with monkeypatch.context() as mp:
        mp.setattr(ss, "loss", _loss_explicit_inverse)
        alt, tr_alt = ss.adam_train(p, X, Y, idx, bb, lr=UNEVEN_LR)
    d = {k: relmax(np.tril(alt[k]), np.tril(ref[k])) if k == "C" else relmax(alt[k], ref[k]) for k in ss.PARAM_NAMES}
    print("CPU formulations: loss trace", f"{relmax(tr_alt, tr_ref):.2e}", {k: f"{v:.1e}" for k, v in d.items()})
    assert relmax(tr_alt, tr_ref) <= 1e-10 and max(d.values()) <= 1e-10
    moved = relmax(ref["C"], p["C"])
    assert moved >= 3e-4, moved             # the steps are 1e5 times the bound: a wrong gradient cannot hide behind the small lr
    tr = _lib.svgp_surface_train(X, Y, p, idx, bb, lr=UNEVEN_LR)
    print("loss trace", f"{relmax(tr, tr_ref):.2e}")
    assert relmax(tr, tr_ref) <= 1e-9
    for k in ss.PARAM_NAMES:
        a, b = (np.tril(p[k]), np.tril(ref[k])) if k == "C" else (p[k], ref[k])
        print(k, f"{relmax(a, b):.2e}")
        assert relmax(a, b) <= 1e-9, k


@pytest.mark.gpu
def test_uneven_batches_in_a_wide_workspace_equal_batches_sized_by_themselves():
    """lr = 0 leaves the parameters as they are (p + (-0) x), so the trace of one training call holds the loss of each
    batch in the workspace sized by the largest one (BP = 1024); gpt_svgp_surface_elbo_grad sizes it by the batch itself.
    Bit for bit: a column of A, U and the statistics is summed over the inducing points only, in an order that does not
    depend on the number of columns (same tile edge 32 at NP = 512 whatever BP: at most 32 tiles), and the residual sums run
    over k < b in the same thread order.  The padding columns must contribute exact zeros."""
    from gaussian_process_transportation_amd import _lib
    X, Y, p, idx, bb = _uneven_schedule()
    q = {k: v.copy() for k, v in p.items()}
    tr = _lib.svgp_surface_train(X, Y, q, idx, bb, lr=0.0)
    for k in ss.PARAM_NAMES:
        a, b = (np.tril(p[k]), np.tril(q[k])) if k == "C" else (p[k], q[k])
        assert np.array_equal(a, b), k
    single = []
    for s in range(len(bb) - 1):
        rows = idx[bb[s]:bb[s + 1]]
        single.append(_lib.svgp_surface_elbo_grad(X[rows], Y[rows], p, len(X))[0])
    print("trace", tr, "single", np.array(single), "difference", tr - np.array(single))
    assert np.array_equal(tr, np.array(single))


def _predict_numpy(p, Xq, explicit_inverse=False):
    """The variational predictive in plain numpy fp64: a = L^-1 c k(Z, x) by a triangular solve, mean a^T m,
    var c - |a|^2 + |C^T a|^2, J_d = sum_i beta_i c k(z_i, x) (z_id - x_d) / l_d^2 with beta = L^-T m.
    explicit_inverse: the same through W = L^-1 formed explicitly (the device's formulation)."""
    Z, T = p["Z"], p["m"].shape[0]
    Zn, D = Z.shape
    mean, var, J = np.empty((len(Xq), T)), np.empty((len(Xq), T)), np.empty((len(Xq), T, D))
    for t in range(T):
        ls, c = _softplus(p["raw_ls"][t]), _softplus(p["raw_os"][t])
        L = np.linalg.cholesky(c * ss_rbf(Z, Z, ls) + EPS * np.eye(Zn))
        kx = c * ss_rbf(Z, Xq, ls)
        if explicit_inverse:
            W = solve_triangular(L, np.eye(Zn), lower=True)
            a, beta = W @ kx, W.T @ p["m"][t]
        else:
            a, beta = solve_triangular(L, kx, lower=True), solve_triangular(L, p["m"][t], lower=True, trans="T")
        Ct = np.tril(p["C"][t])
        mean[:, t] = a.T @ p["m"][t]
        var[:, t] = c - (a * a).sum(0) + ((Ct.T @ a) ** 2).sum(0)
        f = beta[:, None] * kx
        for d in range(D):
            J[:, t, d] = ((Z[:, d][:, None] - Xq[:, d][None, :]) * f).sum(0) / ls[d] ** 2
    return mean, var, J


PREDICT_M = [1, 63, 64, 1023, 1024, 1025, 2500]
_PREDICT_MODELS = {}


def _predict_model(Zn):
    """(params, Xq (2500, D), reference (mean, var, J), tolerances): T = 3, distinct length-scales, random lower C.
    The tolerances are 1e-9 (mean and J of the array scale; var, a difference of O(c) terms, absolute against max c_t),
    widened to 10 d where d, the CPU disagreement of the explicit-inverse formulation with the solve-based one, is above
    1e-10; 10 d <= 1e-7 is asserted (two digits at the most)."""
    if Zn not in _PREDICT_MODELS:
        D = 2 if Zn == 300 else 3
        X, _, p = _problem(Zn, 3, D, Zn + 50, seed=Zn, distinct=True)
        assert np.ptp(p["raw_ls"], axis=0).min() > 0
        Xq = np.random.default_rng(Zn + 1).uniform(-0.05, 1.05, (2500, D))
        ref = _predict_numpy(p, Xq)
        inv = _predict_numpy(p, Xq, explicit_inverse=True)
        cmax = _softplus(p["raw_os"]).max()
        d = (relmax(inv[0], ref[0]), np.abs(inv[1] - ref[1]).max() / cmax, relmax(inv[2], ref[2]))
        print(f"Z {Zn}: explicit inverse against solve: mean {d[0]:.1e} var {d[1]:.1e} J {d[2]:.1e}")
        assert 10 * max(d) <= 1e-7, d
        _PREDICT_MODELS[Zn] = p, Xq, ref, tuple(max(1e-9, 10 * x) for x in d), cmax
    return _PREDICT_MODELS[Zn]


def _predict_errors(got, ref, cmax):
    return relmax(got[0], ref[0]), float(np.abs(got[1] - ref[1]).max() / cmax), relmax(got[2], ref[2])


@pytest.mark.gpu
@pytest.mark.parametrize("M", PREDICT_M)
@pytest.mark.parametrize("Zn", [300, 2200])
def test_predict_chunk_boundaries_match_numpy(Zn, M):
    """Queries below, at and above the 1024-query chunk, and several chunks plus a tail, T = 3."""
    from gaussian_process_transportation_amd import _lib
    p, Xq, ref, tol, cmax = _predict_model(Zn)
    got = _lib.svgp_surface_predict(p, Xq[:M], var=True, J=True)
    err = _predict_errors(got, [r[:M] for r in ref], cmax)
    print(f"Z {Zn} M {M}: mean {err[0]:.2e} var {err[1]:.2e} J {err[2]:.2e} (bounds {tol[0]:.1e} {tol[1]:.1e} {tol[2]:.1e})")
    for e, bound, what in zip(err, tol, ("mean", "var", "J")):
        assert e <= bound, what


@pytest.mark.gpu
@pytest.mark.parametrize("Zn", [300, 2200])
def test_predict_without_var_or_J_returns_the_same_mean(Zn):
    from gaussian_process_transportation_amd import _lib
    p, Xq, ref, tol, cmax = _predict_model(Zn)
    full = _lib.svgp_surface_predict(p, Xq[:1025], var=True, J=True)
    for var, J in ((False, False), (True, False), (False, True)):
        got = _lib.svgp_surface_predict(p, Xq[:1025], var=var, J=J)
        assert np.array_equal(got[0], full[0]), (var, J)
        assert (got[1] is None) == (not var) and (got[2] is None) == (not J)
        if var:
            assert np.array_equal(got[1], full[1])
        if J:
            assert np.array_equal(got[2], full[2])
    # the paths without var / J against the reference too, not only against each other
    assert relmax(full[0], ref[0][:1025]) <= tol[0]


@pytest.mark.gpu
@pytest.mark.parametrize("Zn", [300, 2200])
def test_predict_slices_agree_with_the_full_call(Zn):
    """Xq[a:b] alone against rows a:b of the 2500-query call, for slices that straddle the chunk boundaries 1024 and 2048
    (the slice runs in a chunk of another width)."""
    from gaussian_process_transportation_amd import _lib
    p, Xq, ref, tol, cmax = _predict_model(Zn)
    full = _lib.svgp_surface_predict(p, Xq, var=True, J=True)
    for a, b in ((1000, 1100), (2040, 2056), (1023, 1025), (900, 2100)):
        part = _lib.svgp_surface_predict(p, Xq[a:b], var=True, J=True)
        err = _predict_errors(part, [f[a:b] for f in full], cmax)
        print(f"Z {Zn} slice {a}:{b}: mean {err[0]:.2e} var {err[1]:.2e} J {err[2]:.2e}")
        assert max(err) <= 1e-12, (a, b)


@pytest.mark.gpu
def test_single_task_matches_the_transport_step():
    """T = 1: per-task and shared length-scales are one model; 50 steps against gpt_svgp_train."""
    from gaussian_process_transportation_amd import _lib
    X, Y, p = _problem(100, 1, 3, 300, seed=5)
    rng = np.random.default_rng(1)
    idx = np.concatenate([rng.permutation(300) for _ in range(2)])
    bb = np.arange(0, 501, 10)
    q = {k: v.copy() for k, v in p.items()}
    q["raw_ls"] = p["raw_ls"][0].copy()
    t1 = _lib.svgp_surface_train(X, Y, p, idx, bb)
    t2 = _lib.svgp_train(X, Y, q, idx, bb)
    assert relmax(t1, t2) <= 1e-9
    q["raw_ls"] = q["raw_ls"][None]
    for k in ss.PARAM_NAMES:
        a, b = (np.tril(p[k]), np.tril(q[k])) if k == "C" else (p[k], q[k])
        print(k, f"{relmax(a, b):.2e}")
        assert relmax(a, b) <= 1e-9, k


@pytest.mark.gpu
def test_adam_matches_torch():
    from gaussian_process_transportation_amd import _lib
    X, Y, p = _problem(200, 2, 2, 400, seed=8)
    rng = np.random.default_rng(2)
    idx = np.concatenate([rng.permutation(400) for _ in range(2)])
    bb = np.arange(0, 501, 10)
    ref, tr_ref = ss.adam_train(p, X, Y, idx, bb)
    tr = _lib.svgp_surface_train(X, Y, p, idx, bb)
    assert relmax(tr, tr_ref) <= 1e-9
    for k in ss.PARAM_NAMES:
        a, b = (np.tril(p[k]), np.tril(ref[k])) if k == "C" else (p[k], ref[k])
        print(k, f"{relmax(a, b):.2e}")
        assert relmax(a, b) <= 1e-9, k


def _optimum(Z, X, Y, ls, c, noise, jittered_cross=False):
    """Optimal whitened q(u) of the full-batch ELBO, l per task: (m (T,Zn), C (T,Zn,Zn), A_t list)."""
    T, Zn = Y.shape[1], len(Z)
    m, C, As = np.empty((T, Zn)), np.empty((T, Zn, Zn)), []
    for t in range(T):
        L = np.linalg.cholesky(c[t] * ss_rbf(Z, Z, ls[t]) + EPS * np.eye(Zn))
        A = L.T.copy() if jittered_cross else solve_triangular(L, c[t] * ss_rbf(Z, X, ls[t]), lower=True)
        P = np.linalg.cholesky(np.eye(Zn) + A @ A.T / noise[t])
        S = cho_solve((P, True), np.eye(Zn))
        S = 0.5 * (S + S.T)
        m[t] = S @ (A @ Y[:, t]) / noise[t]
        C[t] = np.linalg.cholesky(S)
        As.append(A)
    return m, C, As


def ss_rbf(a, b, ls):
    d = (a[:, None, :] - b[None, :, :]) / ls
    return np.exp(-0.5 * (d * d).sum(-1))


def _softplus(x):
    return np.log1p(np.exp(x))


def _softplus_inv(x):
    return np.log(np.expm1(np.asarray(x, np.float64)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(40, 120, 3, 2), (300, 600, 2, 3)], ids=lambda c: "Z%d_N%d_T%d_D%d" % c)
def test_titsias_optimum_with_distinct_lengthscales(case):
    """At the closed-form optimal q(u) (full batch) the m and C gradients vanish and the loss is the collapsed bound."""
    from gaussian_process_transportation_amd import _lib
    Zn, N, T, D = case
    rng = np.random.default_rng(Zn + N)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([0.3 * np.sin(3 * X @ rng.standard_normal(D) / np.sqrt(D) + t) for t in range(T)], 1)
    Y = Y + 0.01 * rng.standard_normal(Y.shape)
    Z = rng.uniform(0, 1, (Zn, D))
    raw = {"raw_ls": rng.uniform(-1.5, -0.5, (T, D)) + np.log(D) / 2, "raw_os": rng.uniform(-1.0, 0.5, T),
           "raw_noise": rng.uniform(-6.0, -3.0, T + 1)}
    ls, c, sp = _softplus(raw["raw_ls"]), _softplus(raw["raw_os"]), _softplus(raw["raw_noise"])
    noise = (ss.NOISE_FLOOR + sp[:T]) + (ss.NOISE_FLOOR + sp[T])
    m, C, As = _optimum(Z, X, Y, ls, c, noise)
    bound = 0.0
    for t in range(T):
        A = As[t]
        Lk = np.linalg.cholesky(A.T @ A + noise[t] * np.eye(N))
        w = solve_triangular(Lk, Y[:, t], lower=True)
        bound += -0.5 * (w @ w) - np.log(np.diag(Lk)).sum() - 0.5 * N * np.log(2 * np.pi)
        bound -= (N * (c[t] + EPS) - np.sum(A * A)) / (2 * noise[t])
    _, g0 = _lib.svgp_surface_elbo_grad(X, Y, dict(Z=Z, m=np.zeros((T, Zn)), C=np.tile(np.eye(Zn), (T, 1, 1)), **raw), N)
    loss, g = _lib.svgp_surface_elbo_grad(X, Y, dict(Z=Z, m=m, C=C, **raw), N)
    rm = np.abs(g["m"]).max() / np.abs(g0["m"]).max()
    rc = np.abs(g["C"]).max() / np.abs(g0["C"]).max()
    rl = abs(loss + bound / N) / abs(bound / N)
    print(f"{case}: grad m ratio {rm:.2e}, grad C ratio {rc:.2e}, loss vs collapsed bound {rl:.2e}")
    assert rm <= 1e-12 and rc <= 1e-12
    assert rl <= 1e-10


def _anchor_model(X, Y, c, ls, noise):
    """Z = X, c_t = c, l_t = ls, the optimal q(u) with the cross-covariance c k(X, X) + eps I and noise - eps."""
    T = Y.shape[1]
    m, C, _ = _optimum(X, X, Y, np.tile(ls, (T, 1)), np.full(T, c), np.full(T, noise - EPS), jittered_cross=True)
    return {"Z": X, "m": m, "C": C, "raw_ls": np.tile(_softplus_inv(ls), (T, 1)), "raw_os": np.full(T, _softplus_inv(c)),
            "raw_noise": np.zeros(T + 1)}


def _model_from(params):
    from gaussian_process_transportation_amd import SurfaceSVGP
    T, D = params["m"].shape[0], params["Z"].shape[1]
    model = SurfaceSVGP(np.zeros((1, D)), np.zeros((1, T)), num_inducing=1)
    model.variational_params_ = params
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synthetic_3d_N64", "synthetic_3d_N256", "synthetic_5d_N200", "synthetic_3d_N1024"])
def test_predict_reproduces_synthetic_fixture(name):
    g = load_golden(name)
    keep = ~np.isnan(g["Y"]).any(axis=1)
    X, Y = g["X"][keep], g["Y"][keep]
    ls = np.broadcast_to(np.atleast_1d(g["length_scale"]), (X.shape[1],)).astype(np.float64)
    s2 = float(g["noise_level"])
    model = _model_from(_anchor_model(X, Y, float(g["constant_value"]), ls, s2 + float(g["alpha"])))
    mean, std = model.predict(g["Xq"], return_std=True)
    J = model.derivative(g["Xq"])
    var = (np.asarray(g["std"]) + np.sqrt(s2)) ** 2 - s2
    errs = relmax(mean, g["mean"]), relmax(std ** 2, var), relmax(J, g["J"])
    print(f"{name}: mean {errs[0]:.2e} var {errs[1]:.2e} J {errs[2]:.2e}")
    assert max(errs) <= 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["letterS_2d"])
def test_predict_reproduces_transport_fixture(name):
    """The residual GP of the golden transport: traj, variance and vel of the reference's transport.  (surface_3d has
    noise 3.2e-5 < eps: the identity's likelihood noise sigma^2 + alpha - eps would be negative, so it cannot be built.)"""
    from gaussian_process_transportation_amd import AffineTransform
    g = load_golden(name)
    aff = AffineTransform(verbose=False).fit(g["source"], g["target"])
    Z = aff.predict(g["source"])
    D = Z.shape[1]
    s2 = float(g["noise_level"])
    ls = np.broadcast_to(np.atleast_1d(g["length_scale"]), (D,)).astype(np.float64)
    model = _model_from(_anchor_model(Z, g["target"] - Z, float(g["constant_value"]), ls, s2 + float(g["alpha"])))
    pos = aff.predict(g["demo"])
    mean, std = model.predict(pos, return_std=True)
    J = model.derivative(pos)
    v = aff.derivative(pos) @ np.asarray(g["delta"])[:, :, None]
    got = dict(traj=pos + mean, var=std ** 2, vel=((np.eye(D) + J) @ v)[:, :, 0])
    exp = dict(traj=g["traj"], var=(np.asarray(g["std"]) + np.sqrt(s2)) ** 2 - s2, vel=g["vel"])
    for k in got:
        print(f"{name} {k}: {relmax(got[k], exp[k]):.2e}")
        assert relmax(got[k], exp[k]) <= 1e-7, k


# The reference's flow (fit_point_could.py: Z = 1000, 20 epochs of minibatches of 10).  RMS residual of
# predict(cloud[:, :2]) against z, over std(z), measured on the GPU with np.random.seed(0); each cloud is held to 1.2x its
# own figure.  For comparison: the constant mean(z) scores 1.0, the untrained model (m = 0, predicts 0) 1.7 - 15.5.
# Only dustbin_cover and pan reach 0.5 in 20 epochs: the noise starts at softplus(0) and is still falling (40 epochs:
# 0.53, 0.29, 0.32, 0.26, 0.57).
RESIDUAL_20_EPOCHS = {"distribution": 0.6669, "dustbin_cover": 0.3018, "pan": 0.4718, "white_towelholder": 0.5149,
                      "wood_plate": 0.6685}
# Parameters after the first 20 steps against the CPU restatement: worst measured 1.5e-6 (C of dustbin_cover), bound 2x.
# With 1000 inducing points drawn from ~500 rows (repeats), K(Z,Z) is near singular, and Adam's g / sqrt(v) turns
# summation-order differences in near-zero gradient components into visible steps; the loss trace holds 1e-8.
PARAMS_20_STEPS_TOL = 3e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUDS)
def test_point_cloud_end_to_end(name):
    from gaussian_process_transportation_amd import SurfaceSVGP, _lib
    from gaussian_process_transportation_amd.svgp_exact import svgp_schedule
    cloud = _cloud(name)
    X, z = cloud[:, :2], cloud[:, 2:3]
    epochs = 20
    np.random.seed(0)
    model = SurfaceSVGP(X, z, num_inducing=1000)
    start = {k: v.copy() for k, v in model.variational_params_.items()}
    state = np.random.get_state()
    order, bb = svgp_schedule(len(X), epochs, 10)
    np.random.set_state(state)
    model.fit(num_epochs=epochs)
    # the first 20 steps against the CPU restatement on the same schedule
    p20 = {k: v.copy() for k, v in start.items()}
    tr20 = _lib.svgp_surface_train(X, z, p20, order, bb[:21])
    ref, tr_ref = ss.adam_train(start, X, z, order, bb, n_steps=20)
    assert relmax(tr20, tr_ref) <= 1e-8
    for k in ss.PARAM_NAMES:
        a, b = (np.tril(p20[k]), np.tril(ref[k])) if k == "C" else (p20[k], ref[k])
        print(f"{name} 20 steps {k}: {relmax(a, b):.2e}")
        assert relmax(a, b) <= PARAMS_20_STEPS_TOL, k
    assert np.array_equal(model.loss_history_[:20], tr20)
    trace = model.loss_history_
    steps = len(bb) - 1
    per_epoch = steps // epochs
    assert len(trace) == steps and np.isfinite(trace).all()
    assert trace[-per_epoch:].mean() < trace[:per_epoch].mean()
    pred = model.predict(X)[:, 0]
    sd = z[:, 0].std()
    rms = np.sqrt(np.mean((pred - z[:, 0]) ** 2))
    rms_zero = np.sqrt(np.mean(z[:, 0] ** 2))
    print(f"{name}: N {len(X)}, loss {trace[:per_epoch].mean():.4f} -> {trace[-per_epoch:].mean():.4f}, "
          f"RMS residual / std(z) {rms / sd:.4f} (m = 0: {rms_zero / sd:.3f}, constant mean: 1)")
    assert rms <= 1.2 * RESIDUAL_20_EPOCHS[name] * sd
    assert rms <= 0.85 * sd and rms <= 0.5 * rms_zero          # clearly better than both trivial predictors


@pytest.mark.gpu
def test_two_fits_are_bit_identical():
    from gaussian_process_transportation_amd import SurfaceSVGP
    cloud = _cloud("pan")
    out = []
    for _ in range(2):
        np.random.seed(3)
        model = SurfaceSVGP(cloud[:, :2], cloud[:, 2:], num_inducing=300).fit(num_epochs=1)
        out.append((model.loss_history_, model.variational_params_, model.predict(cloud[:50, :2], return_std=True)))
    assert np.array_equal(out[0][0], out[1][0])
    for k in ss.PARAM_NAMES:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    assert np.array_equal(out[0][2][0], out[1][2][0]) and np.array_equal(out[0][2][1], out[1][2][1])


@pytest.mark.gpu
def test_not_positive_definite_names_the_step_and_leaves_parameters():
    """Two identical inducing points and c = 2^100: c + 1e-4 rounds to c, so chol meets the exact pivot
    c - (c / sqrt(c))^2 = 0 at row 1 of task 1 in the first step (every operation is exact on powers of two)."""
    from gaussian_process_transportation_amd import _lib
    lib = _lib.load()
    X, Y, p = _problem(20, 2, 2, 60, seed=9)
    p["Z"][1] = p["Z"][0]
    p["raw_os"][1] = 2.0 ** 100
    p = {k: np.ascontiguousarray(v, np.float64) for k, v in p.items()}
    before = {k: v.copy() for k, v in p.items()}
    idx = np.arange(60, dtype=np.int64)
    bb = np.array([0, 10, 20], dtype=np.int64)
    trace = np.zeros(2)
    ip = ctypes.POINTER(ctypes.c_int64)
    rc = lib.gpt_svgp_surface_train(0, _lib.dptr(X), _lib.dptr(Y), 60, 2, 2, 20, *(_lib.dptr(p[k]) for k in ss.PARAM_NAMES),
                                    idx.ctypes.data_as(ip), 60, bb.ctypes.data_as(ip), 2, 0.01, _lib.dptr(trace))
    msg = _lib.last_error()
    assert rc == _lib.GPT_E_NOT_PD, (rc, msg)
    assert "optimiser step 0" in msg and "task 1" in msg, msg
    for k in ss.PARAM_NAMES:
        assert np.array_equal(p[k], before[k]), k
    with pytest.raises(np.linalg.LinAlgError, match="optimiser step 0"):
        _lib.svgp_surface_train(X, Y, before, idx, bb)
