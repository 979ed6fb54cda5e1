"""Variational training of the SVGP transport model (gpt_svgp_train / gpt_svgp_elbo_grad, svgp_exact.py): the fp64
restatement of the objective (tests/svgp_elbo_restatement.py) and the pseudo-point conversion on the CPU; the fused HIP
step against autograd and torch.optim.Adam, determinism, argument refusals and the reference's 3-D SVGP example on the GPU.
PARITY WITH GPYTORCH UNPINNED (not available): the restatement is this repository's reading of its defaults."""
import os
import re

import numpy as np
import pytest

from tests import svgp_elbo_restatement as sr
from tests.conftest import ROOT, load_golden, relmax

EPS = sr.JITTER


def _problem(Zn, T, D, N, seed=0, duplicates=False, random_state=True):
    """Smooth multi-output data on [0,1]^D, inducing points from the data (with repeats if asked), and — with
    random_state — a random lower-triangular C and non-zero raw hyper-parameters."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([0.3 * np.sin(3 * X @ rng.standard_normal(D) / np.sqrt(D) + t) for t in range(T)], 1)
    idx = rng.choice(N, Zn, replace=True) if duplicates else rng.permutation(N)[:Zn] if Zn <= N else rng.choice(N, Zn)
    p = sr.init_params(X, Y, idx)
    if duplicates:
        assert len(np.unique(idx)) < Zn
    if random_state:
        p["C"] = np.tril(0.05 * rng.standard_normal((T, Zn, Zn)), -1) + np.eye(Zn) * rng.uniform(0.5, 1.0, (T, 1, Zn))
        p["m"] = p["m"] + 0.1 * rng.standard_normal((T, Zn))
        p["raw_ls"] = rng.uniform(-1.5, -0.5, D) + np.log(D) / 2
        p["raw_os"] = rng.uniform(-1.0, 0.5, T)
        p["raw_noise"] = rng.uniform(-6.0, -3.0, T + 1)
    return X, Y, p


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_restatement_kl_matches_closed_form():
    """The loss is lik + KL / num_data: two num_data values isolate the KL, which must equal the numpy closed form."""
    X, Y, p = _problem(12, 3, 2, 40, seed=3)
    l1, _ = sr.loss_and_grad(p, X[:10], Y[:10], 40)
    l2, _ = sr.loss_and_grad(p, X[:10], Y[:10], 400)
    kl = (l1 - l2) / (1 / 40 - 1 / 400)
    ref = sum(sr.kl_numpy(p["m"][t], p["C"][t]) for t in range(3))
    assert abs(kl - ref) <= 1e-9 * abs(ref)


def _random_q(Zn, T, smax, seed):
    rng = np.random.default_rng(seed)
    C = np.empty((T, Zn, Zn))
    for t in range(T):
        V = np.linalg.qr(rng.standard_normal((Zn, Zn)))[0]
        S = (V * rng.uniform(0.05, smax, Zn)) @ V.T
        C[t] = np.linalg.cholesky(S)
    return C, rng.standard_normal((T, Zn))


@pytest.mark.parametrize("floor,tol,smax", [(0.0, 1e-9, 0.95), (None, 1e-3, 0.95), (None, 1e-3, 0.999)])
def test_pseudo_point_conversion_is_an_identity(floor, tol, smax):
    """For S_t < I the exact GP on (Z, Sigma_t, y_t) is the SVGP predictive: mean A^T m and variance (minus eps)
    c + a^T (S - I) a — exactly without the conversion's floor, within 1e-3 with the shipped one."""
    from gaussian_process_transportation_amd.svgp_exact import PSEUDO_POINT_FLOOR, variational_to_pseudo_points
    from oracle import gp_oracle as orc
    Zn, T, D = 40, 3, 2
    rng = np.random.default_rng(11)
    p = {"Z": rng.uniform(0, 1, (Zn, D)), "raw_ls": np.array([-1.2, -0.9]), "raw_os": np.array([-0.5, 0.0, 0.3]),
         "raw_noise": np.zeros(T + 1)}
    p["C"], p["m"] = _random_q(Zn, T, smax, 5)
    pp = variational_to_pseudo_points(p["Z"], p["m"], p["C"], p["raw_ls"], p["raw_os"],
                                      floor=PSEUDO_POINT_FLOOR if floor is None else floor)
    x = rng.uniform(-0.1, 1.1, (200, D))
    mean, var = sr.whitened_predictive(p, x)
    m2, s2, _, _ = orc.svgp_exact_oracle(x, pp["x_inducing"], pp["var_inducing"], pp["y_inducing"], pp["outputscale"],
                                          pp["lengthscale"])
    assert relmax(m2, mean) <= tol
    assert relmax(s2 ** 2, var - EPS) <= tol


def test_pseudo_point_conversion_stays_positive_definite_past_s_equal_identity():
    """Trained models have eigenvalues of S_t above 1 (the reference's 3-D example: about a third of them); the
    converted c k(Z,Z) + Sigma_t must stay positive definite (gpt_fit_svgp factors it) and keep the mean exact."""
    from gaussian_process_transportation_amd.svgp_exact import variational_to_pseudo_points
    from oracle import gp_oracle as orc
    Zn, T, D = 30, 2, 2
    rng = np.random.default_rng(2)
    p = {"Z": rng.uniform(0, 1, (Zn, D)), "raw_ls": np.array([-1.0, -1.0]), "raw_os": np.array([0.0, -1.0]),
         "raw_noise": np.zeros(T + 1)}
    p["C"], p["m"] = _random_q(Zn, T, 1.8, 9)
    pp = variational_to_pseudo_points(p["Z"], p["m"], p["C"], p["raw_ls"], p["raw_os"])
    ls = pp["lengthscale"]
    R = np.exp(-0.5 * (((p["Z"][:, None] - p["Z"][None]) / ls) ** 2).sum(-1))
    for t in range(T):
        np.linalg.cholesky(pp["outputscale"][t] * R + pp["var_inducing"][t])
    x = rng.uniform(0, 1, (100, D))
    mean, _ = sr.whitened_predictive(p, x)
    assert relmax(orc.svgp_exact_oracle(x, pp["x_inducing"], pp["var_inducing"], pp["y_inducing"], pp["outputscale"],
                                        pp["lengthscale"])[0], mean) <= 1e-9


def test_restatement_adam_lowers_the_full_data_loss():
    """Sanity of the specification: 100 torch-Adam steps of the restatement on a smooth toy problem lower the loss of the
    whole data set."""
    from gaussian_process_transportation_amd.svgp_exact import svgp_schedule
    X, Y, p = _problem(15, 2, 2, 100, seed=1, random_state=False)
    np.random.seed(0)
    idx, bb = svgp_schedule(100, 10)
    before, _ = sr.loss_and_grad(p, X, Y, 100)
    q, trace = sr.adam_train(p, X, Y, idx, bb)
    after, _ = sr.loss_and_grad(q, X, Y, 100)
    assert len(trace) == 100 and after < before - 0.5


def test_schedule_is_the_reference_dataloader():
    """svgp_schedule: a fresh numpy permutation per epoch, batches of 10 with a short last one."""
    from gaussian_process_transportation_amd.svgp_exact import svgp_schedule
    np.random.seed(4)
    idx, bb = svgp_schedule(25, 3)
    np.random.seed(4)
    assert np.array_equal(idx, np.concatenate([np.random.permutation(25) for _ in range(3)]))
    assert np.array_equal(np.diff(bb), [10, 10, 5] * 3) and bb[0] == 0 and bb[-1] == 75


def test_header_declares_the_training_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpt_hip.h")).read(), flags=re.S)
    for name in ("gpt_svgp_train", "gpt_svgp_elbo_grad"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name


def test_variational_training_switch_and_refusal():
    """Both classes take `variational_training`; off (the default) the fit refuses and names the switch."""
    from gaussian_process_transportation_amd import SVGPTransport, StocasticVariationalGaussianProcess
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (30, 2))
    sv = StocasticVariationalGaussianProcess(X, X ** 2, num_inducing=5, variational_training=False)
    with pytest.raises(NotImplementedError, match="variational_training"):
        sv.fit(num_epochs=1)
    assert StocasticVariationalGaussianProcess(X, X, num_inducing=5, variational_training=True).variational_training
    tr = SVGPTransport(verbose=False, variational_training=False)
    tr.source_distribution, tr.target_distribution = X, X + 0.1
    with pytest.raises(NotImplementedError, match="variational_training"):
        tr.fit_transportation(num_epochs=1, num_inducing=5)
    assert SVGPTransport(verbose=False, variational_training=True).variational_training


# ---------------------------------------------------------------------------------------------------------------- GPU

GRAD_CASES = [(5, 2, 1, 10, False), (100, 3, 3, 10, False), (100, 3, 3, 7, False), (200, 2, 15, 64, False),
              (512, 1, 2, 10, False), (60, 2, 3, 10, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("Zn,T,D,b,dup", GRAD_CASES)
def test_elbo_gradient_matches_autograd(Zn, T, D, b, dup):
    """gpt_svgp_elbo_grad: the loss and every raw gradient against autograd of the restatement (fp64), at a random
    lower-triangular C, non-zero raw parameters, a short batch and repeated inducing points."""
    from gaussian_process_transportation_amd import _lib
    N = max(2 * Zn, 300)
    X, Y, p = _problem(Zn, T, D, N, seed=Zn + D + b, duplicates=dup)
    rows = np.random.default_rng(1).choice(N, b, replace=False)
    loss, g = _lib.svgp_elbo_grad(X[rows], Y[rows], p, N)
    rl, rg = sr.loss_and_grad(p, X[rows], Y[rows], N)
    errs = {k: relmax(g[k], rg[k]) for k in sr.PARAM_NAMES}
    print(f"Z={Zn} T={T} D={D} b={b} dup={dup}: loss {abs(loss - rl) / abs(rl):.2e}",
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert abs(loss - rl) <= 1e-9 * abs(rl)
    for k, v in errs.items():
        assert v <= 1e-9, (k, v)
    assert np.all(np.triu(g["C"], 1) == 0)


@pytest.mark.gpu
def test_fifty_adam_steps_match_torch_adam():
    """gpt_svgp_train for 50 steps on a fixed schedule against torch.optim.Adam on the restatement."""
    from gaussian_process_transportation_amd import _lib
    from gaussian_process_transportation_amd.svgp_exact import svgp_schedule
    X, Y, p = _problem(20, 2, 2, 100, seed=7)
    np.random.seed(3)
    idx, bb = svgp_schedule(100, 5)
    assert len(bb) == 51
    ref, rtrace = sr.adam_train(p, X, Y, idx, bb)
    q = {k: v.copy() for k, v in p.items()}
    trace = _lib.svgp_train(X, Y, q, idx, bb, lr=0.01)
    assert relmax(trace, rtrace) <= 1e-9
    for k in sr.PARAM_NAMES:
        assert relmax(q[k], ref[k]) <= 1e-7, (k, relmax(q[k], ref[k]))


@pytest.mark.gpu
def test_fit_is_bit_reproducible():
    from gaussian_process_transportation_amd import StocasticVariationalGaussianProcess
    X, Y, _ = _problem(10, 3, 3, 400, seed=5)
    out = []
    for _ in range(2):
        np.random.seed(12)
        sv = StocasticVariationalGaussianProcess(X, Y, num_inducing=50, dtype="float64", variational_training=True)
        sv.fit(num_epochs=2)
        out.append((sv.variational_params_, sv.loss_history_))
        sv.gp.close()
    for k in sr.PARAM_NAMES:
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    assert np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_refusals():
    from gaussian_process_transportation_amd import _lib
    X, Y, p = _problem(10, 2, 2, 50)
    idx, bb = np.arange(50), np.array([0, 10, 20])
    with pytest.raises(ValueError, match="empty schedule"):
        _lib.svgp_train(X, Y, dict(p), idx, np.array([0]))
    for Zn, T, D in ((1025, 1, 2), (10, 2, 16), (10, 33, 2)):
        Xb, Yb, q = _problem(10, T, D, 50, random_state=False)
        if Zn != 10:
            q["Z"] = np.resize(q["Z"], (Zn, D)); q["m"] = np.zeros((T, Zn)); q["C"] = np.tile(np.eye(Zn), (T, 1, 1))
        with pytest.raises(ValueError):
            _lib.svgp_train(Xb, Yb, q, idx, bb)
    with pytest.raises(ValueError):
        _lib.svgp_train(X, Y, dict(p), np.full(50, 50), bb)             # index out of range


@pytest.mark.gpu
def test_reference_3d_svgp_example_trains_and_transports():
    """example/3D/torch/surface_generalization_3D_svgp.py:41-46 with np.random.seed(0): fit_transportation(num_epochs=10,
    num_inducing=100) on the surface_3d data, then apply_transportation.  The fp64 CPU restatement with this seed went from
    a first-epoch mean loss of 1.63 to -7.79 and transported within 4.2 % (max) / 1.4 % (mean) of the displacement of the
    exact GP's golden trajectory."""
    from gaussian_process_transportation_amd import SVGPTransport
    g = load_golden("surface_3d")
    np.random.seed(0)
    tr = SVGPTransport(verbose=False, variational_training=True)
    tr.source_distribution, tr.target_distribution = g["source"], g["target"]
    tr.training_traj = g["demo"]
    tr.fit_transportation(num_epochs=10, num_inducing=100)
    tr.apply_transportation()
    hist = tr.gp_delta_map.loss_history_.reshape(10, -1).mean(1)
    print("epoch mean loss", np.round(hist, 3))
    assert hist[-1] < hist[0]
    disp = np.linalg.norm(g["traj"] - g["demo"], axis=1)
    err = np.linalg.norm(tr.training_traj - g["traj"], axis=1)
    print(f"trajectory error: max {err.max() / disp.max():.3%} of the largest displacement, mean {err.mean() / disp.mean():.3%}")
    assert err.max() <= 0.08 * disp.max() and err.mean() <= 0.03 * disp.mean()
    mean, _ = sr.whitened_predictive(tr.gp_delta_map.variational_params_, tr.traj_rotated)
    assert relmax(tr.delta_map_mean, mean) <= 5e-3
