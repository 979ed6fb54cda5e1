"""The SVGP path anchored to numbers of the reference (tests/golden/*.npz) and to closed-form identities, not to this
repository's restatements alone.  Three identities tie the SVGP algebra to them:

1. Homoscedastic reduction.  The exact-conversion model with Z = X, Sigma_t = (sigma^2 + alpha) I, y_t = Y[:, t],
   outputscale_t = c and the fixture's length-scale IS the fixture's sklearn GP.  Golden `std` is
   sqrt(c + sigma^2 - q) - sqrt(sigma^2) (the reference's quirk), so the SVGP variance c - q is
   (std + sqrt(sigma^2))^2 - sigma^2; golden `Jvar` and `dvar` are variances / derivatives of the variance.
2. Optimal q(u).  For fixed hyper-parameters and a full batch the whitened ELBO is maximised by
   S_t = (I + A_t A_t^T / noise_t)^-1, m_t = S_t A_t y_t / noise_t with A_t = L_t^-1 K_t(Z, X) and
   L_t = chol(c_t k(Z, Z) + eps I).  With Z = X, K_t(Z, X) = c_t k(X, X) + eps I (so A_t = L_t^T: the data see f_X = L_t u,
   the jittered prior the pseudo-point conversion assumes) and noise_t = sigma^2 + alpha - eps, this q(u) is the exact
   posterior of the fixture's GP, and `variational_to_pseudo_points` of it must predict what the fixture predicts.
   (With the un-jittered cross-covariance c_t k(X, X), as the training kernel uses, the optimum is the DTC posterior: its
   mean differs from the exact GP's by O(eps / lambda) in the directions of eigenvalue lambda of c_t k(X, X), measured
   9e-4 on synthetic_3d_N64, so it is no identity.)
3. Stationary point.  At that optimum (any Z) the gradients of the negative ELBO in m and C vanish and the loss equals
   the collapsed (Titsias) bound, -(1/N) sum_t [log N(y_t | 0, A_t^T A_t + noise_t I) - (N (c_t + eps) - tr A_t^T A_t)
   / (2 noise_t)], computed here in numpy fp64.

CPU tests check the identities on the restatements (oracle/gp_oracle.py, tests/svgp_elbo_restatement.py); GPU tests
check the HIP kernels (gpt_fit_svgp and the stacked-task k_mean_jac / k_var, gpt_svgp_elbo_grad) through them.  Bounds:
1e-9 on the CPU, 1e-7 per array (max-norm relative) for fp64 on the GPU; fp32 models may lose no more than the same
algebra restated in numpy float32, or 2e-4."""
import numpy as np
import pytest
from scipy.linalg import cho_solve, solve_triangular

from tests import svgp_elbo_restatement as sr
from tests.conftest import assert_parity, load_golden, relmax

EPS = sr.JITTER
CPU_TOL = 1e-9
GPU_TOL = 1e-7
SYN = ["synthetic_3d_N64", "synthetic_3d_N64_iso", "synthetic_3d_N64_nan", "synthetic_3d_N256", "synthetic_3d_N1024",
       "synthetic_5d_N200", "synthetic_8d_N128", "synthetic_12d_N160", "synthetic_15d_N96"]
SMALL = ["synthetic_3d_N64", "synthetic_3d_N64_iso", "synthetic_3d_N64_nan", "synthetic_8d_N128", "synthetic_15d_N96"]
MAX_TASKS = 32


def _softplus_inv(x):
    return np.log(np.expm1(np.asarray(x, np.float64)))


def _rbf(a, b, ls):
    d = (a[:, None, :] - b[None, :, :]) / ls
    return np.exp(-0.5 * (d * d).sum(-1))


# ------------------------------------------------------------------------------------------- identity 1: the fixtures

def _homoscedastic(g):
    """(X, Y, c, ls (D,), sigma^2, sigma^2 + alpha) of a synthetic fixture, NaN rows of Y dropped as the reference does."""
    keep = ~np.isnan(g["Y"]).any(axis=1)
    X, Y = g["X"][keep], g["Y"][keep]
    ls = np.broadcast_to(np.atleast_1d(g["length_scale"]), (X.shape[1],)).astype(np.float64)
    s2 = float(g["noise_level"])
    return X, Y, float(g["constant_value"]), ls, s2, s2 + float(g["alpha"])


def _golden_var(std, s2):
    """The SVGP variance c - q from the reference's std = sqrt(c + sigma^2 - q) - sqrt(sigma^2)."""
    return (np.asarray(std) + np.sqrt(s2)) ** 2 - s2


def _expected(g):
    """Golden mean (M,O), variance (M,O), J (M,O,D), Jacobian variance (M,O,D), d variance (D,M)."""
    _, _, _, _, s2, _ = _homoscedastic(g)
    return g["mean"], _golden_var(g["std"], s2), g["J"], g["Jvar"], g["dvar"]


def _pseudo_points(g):
    """Identity 1: keyword arguments of set_pseudo_points / the oracle for the fixture's GP, one task per output."""
    X, Y, c, ls, _, nv = _homoscedastic(g)
    O, N = Y.shape[1], len(X)
    return dict(x_inducing=X, var_inducing=np.tile(nv * np.eye(N), (O, 1, 1)), y_inducing=Y.T.copy(),
                outputscale=np.full(O, c), lengthscale=ls)


def _oracle(x, pp, dtype=np.float64):
    from oracle import gp_oracle as orc
    return orc.svgp_exact_oracle_fast(x, pp["x_inducing"], pp["var_inducing"], pp["y_inducing"], pp["outputscale"],
                                      pp["lengthscale"], dtype=dtype)


def _check_predictive(tag, got, exp, tol):
    """got = (mean, var, J, Jvar) against the golden (mean, var, J, Jvar); prints and asserts each array."""
    for name, a, b in zip(("mean", "var", "J", "Jvar"), got, exp):
        err = relmax(a, b)
        print(f"{tag} {name}: {err:.2e}")
        assert_parity(a, b, tol, f"{tag} {name}")


TRANSPORT = {"letterS_2d": "letter-S", "surface_3d": "surface-3D"}


def _transport_case(name):
    """Identity 1 for a transport fixture: the affine pre-alignment (Z = aligned source = golden gp_X where stored),
    the pseudo-points of the exact GP on the residual and the golden traj / variance / vel / var_vel."""
    from gaussian_process_transportation_amd import AffineTransform
    g = load_golden(name)
    aff = AffineTransform(verbose=False).fit(g["source"], g["target"])
    Z = aff.predict(g["source"])
    if "gp_X" in g:
        assert relmax(Z, g["gp_X"]) <= 1e-12
    T = Z.shape[1]
    s2 = float(g["noise_level"])
    nv = s2 + float(g["alpha"])
    ls = np.broadcast_to(np.atleast_1d(g["length_scale"]), (T,)).astype(np.float64)
    pp = dict(x_inducing=Z, var_inducing=np.tile(nv * np.eye(len(Z)), (T, 1, 1)),
              y_inducing=(g["target"] - Z).T.copy(), outputscale=np.full(T, float(g["constant_value"])), lengthscale=ls)
    exp = dict(traj=g["traj"], var=_golden_var(g["std"], s2), vel=g["vel"], var_vel=g["var_vel"])
    return g, aff, pp, exp


def _transport_from_posterior(aff, demo, delta, mean, std, J, Jstd):
    """policy_transportation's algebra (the SVGP transport's apply_transportation) on given posterior arrays."""
    pos = aff.predict(demo)
    v = aff.derivative(pos) @ np.asarray(delta)[:, :, None]
    return dict(traj=pos + mean, var=np.asarray(std, np.float64) ** 2, vel=((np.eye(pos.shape[1]) + J) @ v)[:, :, 0],
                var_vel=(np.asarray(Jstd, np.float64) ** 2 @ v ** 2)[:, :, 0])


# ------------------------------------------------------------------------------------------- identity 2: optimal q(u)

def _titsias_optimum(Z, X, Y, ls, c, noise, jittered_cross=False):
    """Optimal whitened q(u) of the full-batch ELBO for fixed hyper-parameters: m (T,Zn), C = chol(S) (T,Zn,Zn).
    jittered_cross (Z = X only): the cross-covariance c k(Z, X) + eps I, so that A = L^T and the data see f_X = L u."""
    T, Zn = Y.shape[1], len(Z)
    Ruu, Rux = _rbf(Z, Z, ls), _rbf(Z, X, ls)
    m = np.empty((T, Zn))
    C = np.empty((T, Zn, Zn))
    for t in range(T):
        L = np.linalg.cholesky(c[t] * Ruu + EPS * np.eye(Zn))
        A = L.T.copy() if jittered_cross else solve_triangular(L, c[t] * Rux, lower=True)
        P = np.linalg.cholesky(np.eye(Zn) + A @ A.T / noise[t])          # S = (P P^T)^-1
        S = cho_solve((P, True), np.eye(Zn))
        S = 0.5 * (S + S.T)
        m[t] = S @ (A @ Y[:, t]) / noise[t]
        C[t] = np.linalg.cholesky(S)
    return m, C


def _identity2_pseudo_points(X, Y, ls, c, noise, floor=None):
    """Identity 2 at Z = X: the optimal q(u) converted by variational_to_pseudo_points (raw = softplus^-1)."""
    from gaussian_process_transportation_amd.svgp_exact import PSEUDO_POINT_FLOOR, variational_to_pseudo_points
    T = Y.shape[1]
    m, C = _titsias_optimum(X, X, Y, ls, np.full(T, c), np.full(T, noise), jittered_cross=True)
    return variational_to_pseudo_points(X, m, C, _softplus_inv(ls), _softplus_inv(np.full(T, c)),
                                        floor=PSEUDO_POINT_FLOOR if floor is None else floor)


# ------------------------------------------------------------------------------------------- identity 3: stationarity

ELBO_CASES = [(24, 60, 3, 3, False), (64, 64, 3, 3, True), (200, 1000, 2, 15, False), (1024, 1024, 1, 2, False),
              (100, 300, 32, 3, False)]


def _elbo_problem(Zn, N, T, D, z_is_x, seed=0):
    """Smooth multi-output data, inducing points (Z = X, or uniform draws), non-zero raw hyper-parameters and per-task
    raw noises; returns X, Y, the parameters at the optimum of q(u), at the start m = 0, C = I, and the closed-form
    collapsed bound (as a loss: minus the bound over N)."""
    rng = np.random.default_rng(seed + Zn + N + T + D)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([0.3 * np.sin(3 * X @ rng.standard_normal(D) / np.sqrt(D) + t) for t in range(T)], 1)
    Y = Y + 0.01 * rng.standard_normal(Y.shape)
    Z = X.copy() if z_is_x else rng.uniform(0, 1, (Zn, D))
    assert len(Z) == Zn
    raw = {"raw_ls": rng.uniform(-1.5, -0.5, D) + np.log(D) / 2, "raw_os": rng.uniform(-1.0, 0.5, T),
           "raw_noise": rng.uniform(-6.0, -3.0, T + 1)}
    ls, c = np.log1p(np.exp(raw["raw_ls"])), np.log1p(np.exp(raw["raw_os"]))
    sp = np.log1p(np.exp(raw["raw_noise"]))
    noise = (sr.NOISE_FLOOR + sp[:T]) + (sr.NOISE_FLOOR + sp[T])
    m, C = _titsias_optimum(Z, X, Y, ls, c, noise)
    opt = dict(Z=Z, m=m, C=C, **raw)
    start = dict(Z=Z, m=np.zeros((T, Zn)), C=np.tile(np.eye(Zn), (T, 1, 1)), **raw)
    Ruu, Rux = _rbf(Z, Z, ls), _rbf(Z, X, ls)
    bound = 0.0
    for t in range(T):
        L = np.linalg.cholesky(c[t] * Ruu + EPS * np.eye(Zn))
        A = solve_triangular(L, c[t] * Rux, lower=True)
        Kt = A.T @ A + noise[t] * np.eye(N)
        Lk = np.linalg.cholesky(Kt)
        w = solve_triangular(Lk, Y[:, t], lower=True)
        logp = -0.5 * (w @ w) - np.log(np.diag(Lk)).sum() - 0.5 * N * np.log(2 * np.pi)
        bound += logp - (N * (c[t] + EPS) - np.sum(A * A)) / (2 * noise[t])
    return X, Y, opt, start, -bound / N


def _check_stationary(tag, evaluate, case):
    Zn, N, T, D, zx = case
    X, Y, opt, start, collapsed = _elbo_problem(*case)
    _, g0 = evaluate(start, X, Y, N)
    loss, g = evaluate(opt, X, Y, N)
    rm = np.abs(g["m"]).max() / np.abs(g0["m"]).max()
    rc = np.abs(np.tril(g["C"])).max() / np.abs(np.tril(g0["C"])).max()
    rl = abs(loss - collapsed) / abs(collapsed)
    print(f"{tag} Zn={Zn} N={N} T={T} D={D} Z=X:{zx}: |grad m| {np.abs(g['m']).max():.2e} (start {np.abs(g0['m']).max():.2e}, "
          f"ratio {rm:.2e}), |grad C| {np.abs(g['C']).max():.2e} (start {np.abs(g0['C']).max():.2e}, ratio {rc:.2e}), "
          f"loss vs collapsed bound {rl:.2e}")
    assert rm <= 1e-9 and rc <= 1e-9, (rm, rc)
    assert rl <= 1e-10, rl


# ========================================================================================================= CPU

@pytest.mark.parametrize("name", SYN)
def test_homoscedastic_svgp_restatement_reproduces_fixture(name):
    """(a) Identity 1 on svgp_exact_oracle_fast (and svgp_exact_oracle on the small fixtures)."""
    from oracle import gp_oracle as orc
    g = load_golden(name)
    pp = _pseudo_points(g)
    mean, var, J, Jvar, _ = _expected(g)
    m, s, Jm, Js = _oracle(g["Xq"], pp)
    _check_predictive(f"{name} oracle_fast", (m, s ** 2, Jm, Js ** 2), (mean, var, J, Jvar), CPU_TOL)
    if name in SMALL:
        m, s, Jm, Js = orc.svgp_exact_oracle(g["Xq"], pp["x_inducing"], pp["var_inducing"], pp["y_inducing"],
                                             pp["outputscale"], pp["lengthscale"])
        _check_predictive(f"{name} oracle", (m, s ** 2, Jm, Js ** 2), (mean, var, J, Jvar), CPU_TOL)


@pytest.mark.parametrize("name", list(TRANSPORT))
def test_homoscedastic_svgp_restatement_reproduces_transport(name):
    """(a) Identity 1 through the transport algebra: traj, variance, vel and var_vel of the golden transport."""
    g, aff, pp, exp = _transport_case(name)
    post = _oracle(aff.predict(g["demo"]), pp)
    got = _transport_from_posterior(aff, g["demo"], g["delta"], *post)
    for k in ("traj", "var", "vel", "var_vel"):
        print(f"{TRANSPORT[name]} oracle_fast {k}: {relmax(got[k], exp[k]):.2e}")
        assert_parity(got[k], exp[k], CPU_TOL, k)


@pytest.mark.parametrize("name", ["synthetic_3d_N64", "synthetic_3d_N256", "letterS_2d"])
@pytest.mark.parametrize("floor", [0.0, None])
def test_optimal_variational_posterior_converts_to_fixture(name, floor):
    """(b) Identity 2: closed-form q* -> variational_to_pseudo_points (with and without its eigenvalue floor) -> the
    exact GP of the fixture."""
    if name in TRANSPORT:
        g, aff, pp, exp = _transport_case(name)
        Z, Y = pp["x_inducing"], pp["y_inducing"].T
    else:
        g = load_golden(name)
        Z, Y, _, _, _, _ = _homoscedastic(g)
    ls = np.broadcast_to(np.atleast_1d(g["length_scale"]), (Z.shape[1],))
    nv = float(g["noise_level"]) + float(g["alpha"])
    pq = _identity2_pseudo_points(Z, Y, ls, float(g["constant_value"]), nv - EPS, floor)
    if name in TRANSPORT:
        got = _transport_from_posterior(aff, g["demo"], g["delta"], *_oracle(aff.predict(g["demo"]), pq))
        for k in ("traj", "var", "vel", "var_vel"):
            print(f"{name} q* floor={floor} {k}: {relmax(got[k], exp[k]):.2e}")
            assert_parity(got[k], exp[k], CPU_TOL, k)
    else:
        m, s, Jm, Js = _oracle(g["Xq"], pq)
        _check_predictive(f"{name} q* floor={floor}", (m, s ** 2, Jm, Js ** 2), _expected(g)[:4], CPU_TOL)


@pytest.mark.parametrize("case", [c for c in ELBO_CASES if c[0] <= 200], ids=lambda c: "Z%d_N%d_T%d_D%d" % c[:4])
def test_restatement_is_stationary_at_the_titsias_optimum(case):
    """(c) Identity 3 on the torch restatement: zero m / C gradients and the collapsed bound at q*."""
    _check_stationary("restatement", sr.loss_and_grad, case)


# ========================================================================================================= GPU fp64

def _fit(Z, y, Sigma, ls, osc, jitter=0.0, dtype=None, handle=None):
    from gaussian_process_transportation_amd import _lib
    h = handle if handle is not None else _lib.Handle(0)
    h.fit_svgp(Z, y, Sigma, ls, osc, jitter=jitter, dtype=_lib.GPT_F64 if dtype is None else dtype)
    return h


def _fit_fixture(g, dtype=None, **kw):
    pp = _pseudo_points(g)
    return _fit(pp["x_inducing"], pp["y_inducing"], pp["var_inducing"], pp["lengthscale"], pp["outputscale"],
                dtype=dtype, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SYN)
def test_stacked_task_handle_reproduces_fixture(name):
    """(d) gpt_fit_svgp with T = O tasks (up to 15 at D = 15) against the fixture's mean / variance / J / Jvar."""
    g = load_golden(name)
    h = _fit_fixture(g)
    assert h.model_info()[0] == g["Y"].shape[1]
    out = h.predict_all(g["Xq"], mean=True, var=True, J=True, Jvar=True)
    _check_predictive(f"{name} gpu f64", (out["mean"], out["var"], out["J"], out["Jvar"]), _expected(g)[:4], GPU_TOL)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synthetic_3d_N64_iso", "synthetic_12d_N160"])
def test_svgp_wrapper_reproduces_fixture(name):
    """(d) The same through StocasticVariationalGaussianProcess.set_pseudo_points / SVGPExactPredictor, where std and
    the Jacobian std are square-rooted."""
    from gaussian_process_transportation_amd import StocasticVariationalGaussianProcess
    g = load_golden(name)
    X, Y, _, _, _, _ = _homoscedastic(g)
    mean, var, J, Jvar, _ = _expected(g)
    sv = StocasticVariationalGaussianProcess(X, Y, dtype="float64").set_pseudo_points(**_pseudo_points(g))
    m, s = sv.predict(g["Xq"], return_std=True)
    Jm, Js = sv.derivative(g["Xq"])
    for tag, a, b in (("mean", m, mean), ("std", s, np.sqrt(var)), ("J", Jm, J), ("J std", Js, np.sqrt(Jvar))):
        print(f"{name} wrapper f64 {tag}: {relmax(a, b):.2e}")
        assert_parity(a, b, GPU_TOL, tag)
    sv.gp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synthetic_3d_N256", "synthetic_5d_N200"])
def test_single_task_handle_returns_golden_dvar(name):
    """(e) One T = 1 handle per output: d variance / dx (defined for one task) against golden dvar."""
    g = load_golden(name)
    X, Y, c, ls, _, nv = _homoscedastic(g)
    mean, var, J, Jvar, dvar = _expected(g)
    for o in range(Y.shape[1]):
        h = _fit(X, Y[:, o][None], nv * np.eye(len(X))[None], ls, np.array([c]))
        out = h.predict_all(g["Xq"], mean=True, var=True, J=True, Jvar=True, dvar=True)
        _check_predictive(f"{name} T=1 output {o}", (out["mean"][:, 0], out["var"], out["J"][:, 0], out["Jvar"]),
                          (mean[:, o], var[:, o], J[:, o], Jvar[:, o]), GPU_TOL)
        print(f"{name} T=1 output {o} dvar: {relmax(out['dvar'], dvar):.2e}")
        assert_parity(out["dvar"], dvar, GPU_TOL, "dvar")
        h.close()


def _scaled_tasks(g, T):
    """T tasks from the fixture's O outputs: task t = output t mod O scaled by s_t (1e-3 .. 1e3, neighbours ~10^3 apart):
    y s_t, outputscale c s_t^2, Sigma s_t^2."""
    X, Y, c, ls, _, nv = _homoscedastic(g)
    e = np.linspace(-3.0, 3.0, MAX_TASKS)
    order = np.empty(MAX_TASKS, dtype=int)
    order[0::2], order[1::2] = np.arange(MAX_TASKS // 2), np.arange(MAX_TASKS // 2, MAX_TASKS)
    s = 10.0 ** e[order][:T]
    out = np.arange(T) % Y.shape[1]
    N = len(X)
    Sigma = (nv * s ** 2)[:, None, None] * np.eye(N)[None]
    return X, (Y[:, out] * s).T.copy(), Sigma, ls, c * s ** 2, s, out


def _check_scaled(tag, res, g, s, out, rows=slice(None)):
    """Each task against its own scale: golden mean / J times s_t, variance / Jvar times s_t^2."""
    mean, var, J, Jvar, _ = _expected(g)
    worst = {k: 0.0 for k in ("mean", "var", "J", "Jvar")}
    for t in range(len(s)):
        o = out[t]
        exp = dict(mean=mean[:, o] * s[t], var=var[:, o] * s[t] ** 2, J=J[:, o] * s[t], Jvar=Jvar[:, o] * s[t] ** 2)
        for k, b in exp.items():
            a = res[k][rows, t]
            worst[k] = max(worst[k], relmax(a, b))
            assert_parity(a, b, GPU_TOL, f"{tag} task {t} (scale {s[t]:.1e}) {k}")
    print(f"{tag}: worst per-task error " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [MAX_TASKS, 5])
def test_task_stacking_keeps_tasks_apart(T):
    """(f) T = 32 (MAX_TASKS) and T = 5 (not a multiple of the 4-column alpha pass) scaled tasks of one handle, each task
    checked against its own scale so that a leak from a 1e3 task into a 1e-3 neighbour fails."""
    g = load_golden("synthetic_3d_N256")
    X, y, Sigma, ls, osc, s, out = _scaled_tasks(g, T)
    h = _fit(X, y, Sigma, ls, osc)
    assert h.model_info()[0] == T
    res = h.predict_all(g["Xq"], mean=True, var=True, J=True, Jvar=True)
    _check_scaled(f"T={T}", res, g, s, out)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synthetic_3d_N256", "synthetic_15d_N96"])
def test_jitter_argument_is_added_once(name):
    """(g) Sigma = (sigma^2 + alpha)/2 I with jitter (sigma^2 + alpha)/2, and Sigma = 0 with jitter sigma^2 + alpha, are the
    model of (d): a dropped or doubled jitter fails."""
    g = load_golden(name)
    X, Y, c, ls, _, nv = _homoscedastic(g)
    O, N = Y.shape[1], len(X)
    osc = np.full(O, c)
    flags = dict(mean=True, var=True, J=True, Jvar=True)
    h = _fit(X, Y.T, np.tile(nv * np.eye(N), (O, 1, 1)), ls, osc)
    ref = h.predict_all(g["Xq"], **flags)
    for tag, Sig, jit in (("half", 0.5 * nv, 0.5 * nv), ("all", 0.0, nv)):
        _fit(X, Y.T, np.tile(Sig * np.eye(N), (O, 1, 1)), ls, osc, jitter=jit, handle=h)
        res = h.predict_all(g["Xq"], **flags)
        errs = {k: relmax(res[k], ref[k]) for k in flags}
        print(f"{name} jitter {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= 1e-12, (tag, k, v)
        _check_predictive(f"{name} jitter {tag}", (res["mean"], res["var"], res["J"], res["Jvar"]), _expected(g)[:4], GPU_TOL)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synthetic_3d_N256", "synthetic_3d_N1024"])
def test_noise_matrix_fit_reproduces_fixture(name):
    """(h) gpt_fit_noise_matrix with Sigma = (sigma^2 + alpha) I, constant c and alpha 0."""
    from gaussian_process_transportation_amd import _lib
    g = load_golden(name)
    X, Y, c, ls, _, nv = _homoscedastic(g)
    mean, var, J, Jvar, dvar = _expected(g)
    h = _lib.Handle(0)
    h.fit_noise_matrix(X, Y, ls, c, nv * np.eye(len(X)), alpha=0.0)
    out = h.predict_all(g["Xq"], mean=True, var=True, J=True, Jvar=True, dvar=True)
    _check_predictive(f"{name} noise matrix", (out["mean"], out["var"], out["J"], out["Jvar"]),
                      (mean, var[:, 0], J, Jvar[:, 0]), GPU_TOL)
    print(f"{name} noise matrix dvar: {relmax(out['dvar'], dvar):.2e}")
    assert_parity(out["dvar"], dvar, GPU_TOL, "dvar")
    h.close()


def _svgp_transport(name, dtype):
    from gaussian_process_transportation_amd import SVGPTransport
    g, aff, pp, exp = _transport_case(name)
    tr = SVGPTransport(dtype=dtype, verbose=False)
    tr.source_distribution, tr.target_distribution = g["source"], g["target"]
    tr.training_traj, tr.training_delta = g["demo"], g["delta"]
    tr.fit_transportation(pseudo_points=pp)
    tr.apply_transportation()
    got = dict(traj=tr.training_traj, std=tr.std, vel=tr.training_delta, var_vel=tr.var_vel_transported)
    tr.gp_delta_map.gp.close()
    return g, aff, pp, exp, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRANSPORT))
def test_svgp_transport_reproduces_golden_transport(name):
    """(i) SVGPTransport (fp64) with the pseudo-points of identity 1: letter-S (Z = 20) and surface-3D (Z = 2500, padded
    past the 512 tiles) against golden traj / vel / var_vel and the converted std."""
    _, _, _, exp, got = _svgp_transport(name, "float64")
    exp = dict(exp, std=np.sqrt(exp["var"]))
    for k, tol in (("traj", 1e-7), ("vel", 1e-7), ("std", 1e-6), ("var_vel", 1e-6)):
        print(f"{TRANSPORT[name]} SVGPTransport f64 {k}: {relmax(got[k], exp[k]):.2e}")
        assert_parity(got[k], exp[k], tol, k)


@pytest.mark.gpu
def test_optimal_variational_posterior_end_to_end():
    """(j) Identity 2 on the GPU: q* -> variational_to_pseudo_points -> set_pseudo_points (fp64) -> the fixture."""
    from gaussian_process_transportation_amd import StocasticVariationalGaussianProcess
    g = load_golden("synthetic_3d_N256")
    X, Y, c, ls, _, nv = _homoscedastic(g)
    mean, var, J, Jvar, _ = _expected(g)
    sv = StocasticVariationalGaussianProcess(X, Y, dtype="float64")
    sv.set_pseudo_points(**_identity2_pseudo_points(X, Y, ls, c, nv - EPS))
    m, s = sv.predict(g["Xq"], return_std=True)
    Jm, Js = sv.derivative(g["Xq"])
    _check_predictive("N256 q* gpu f64", (m, s ** 2, Jm, Js ** 2), (mean, var, J, Jvar), GPU_TOL)
    sv.gp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ELBO_CASES, ids=lambda c: "Z%d_N%d_T%d_D%d" % c[:4])
def test_elbo_kernel_is_stationary_at_the_titsias_optimum(case):
    """(k) Identity 3 on gpt_svgp_elbo_grad with a full batch: zero m / C gradients and the collapsed bound at q*."""
    from gaussian_process_transportation_amd import _lib
    _check_stationary("gpu", lambda p, X, Y, n: _lib.svgp_elbo_grad(X, Y, p, n), case)


@pytest.mark.gpu
def test_device_group_shards_the_stacked_task_model():
    """(l) DeviceGroup([0, 0]).fit_svgp with the T = 32 model of (f) on 4096 query rows (two shards of the multi-task blob):
    mean and J bit-identical to one handle, var and Jvar within 1e-11 per task, the golden rows checked as in (f)."""
    from gaussian_process_transportation_amd.device_group import DeviceGroup
    g = load_golden("synthetic_3d_N256")
    X, y, Sigma, ls, osc, s, out = _scaled_tasks(g, MAX_TASKS)
    nq = len(g["Xq"])
    Xq = np.concatenate([g["Xq"], np.random.default_rng(7).uniform(-0.1, 1.1, (4096 - nq, 3))])
    flags = dict(mean=True, var=True, J=True, Jvar=True)
    h = _fit(X, y, Sigma, ls, osc)
    ref = h.predict_all(Xq, **flags)
    grp = DeviceGroup([0, 0])
    try:
        grp.fit_svgp(X, y, Sigma, ls, osc)
        assert len(grp.shards(len(Xq))) == 2
        res = grp.predict_all(Xq, **flags)
    finally:
        grp.close()
    assert np.array_equal(res["mean"], ref["mean"]) and np.array_equal(res["J"], ref["J"])
    worst = max(max(relmax(res[k][:, t], ref[k][:, t]) for t in range(MAX_TASKS)) for k in ("var", "Jvar"))
    print(f"DeviceGroup T=32: var / Jvar vs one handle, worst per-task {worst:.2e}")
    assert worst <= 1e-11
    _check_scaled("DeviceGroup T=32 golden rows", res, g, s, out, rows=slice(0, nq))
    h.close()


# ========================================================================================================= GPU fp32

def _fp32_rule(tag, got, exp, ref32):
    """fp32 model: error against the golden <= max(2e-4, the error of the numpy float32 restatement)."""
    for k in exp:
        err, err32 = relmax(got[k], exp[k]), relmax(ref32[k], exp[k])
        print(f"{tag} {k}: GPU {err:.2e}, numpy float32 restatement {err32:.2e}")
        assert np.all(np.isfinite(got[k])), k
        assert err <= max(2e-4, err32), (k, err, err32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SYN)
def test_stacked_task_handle_fp32_model(name):
    """(m) fp32 variant of (d), compared as mean / std / J / J std."""
    from gaussian_process_transportation_amd import _lib
    g = load_golden(name)
    h = _fit_fixture(g, dtype=_lib.GPT_F32)
    out = h.predict_all(g["Xq"], mean=True, var=True, J=True, Jvar=True)
    assert out["mean"].dtype == np.float32
    mean, var, J, Jvar, _ = _expected(g)
    exp = dict(mean=mean, std=np.sqrt(var), J=J, Jstd=np.sqrt(Jvar))
    got = dict(mean=out["mean"], std=np.sqrt(np.maximum(out["var"].astype(np.float64), 0)), J=out["J"],
               Jstd=np.sqrt(np.maximum(out["Jvar"].astype(np.float64), 0)))
    r = _oracle(g["Xq"], _pseudo_points(g), dtype=np.float32)
    _fp32_rule(f"{name} gpu f32", got, exp, dict(zip(("mean", "std", "J", "Jstd"), r)))
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRANSPORT))
def test_svgp_transport_fp32_model(name):
    """(m) fp32 variant of (i)."""
    g, aff, pp, exp, got = _svgp_transport(name, "float32")
    exp = dict(exp, std=np.sqrt(exp["var"]))
    del exp["var"]
    r = _transport_from_posterior(aff, g["demo"], g["delta"], *_oracle(aff.predict(g["demo"]), pp, dtype=np.float32))
    r["std"] = np.sqrt(r.pop("var"))
    _fp32_rule(f"{TRANSPORT[name]} SVGPTransport f32", got, exp, r)
