"""Posterior derivatives of Matern 3/2 and 5/2 models (GaussianProcess(..., matern_derivatives=True)).

The reference has no number to match here (it multiplies the Matern k* by the RBF coefficient), so the target is the
analytic derivative of the Matern posterior, written out in numpy below:
    r = |(x - X_n) / l|,  u_d = (X_n,d - x_d) / l_d^2,  d k(x, X_n) / d x_d = c g(r) u_d
    Matern 3/2: g = 3 e^{-sqrt3 r}          Matern 5/2: g = 5/3 (1 + sqrt5 r) e^{-sqrt5 r}
    J[m,o,d] = sum_n dk_d[m,n] alpha[n,o];  Jvar[m,d] = c g(0) / l_d^2 - dk_d^T K^-1 dk_d;  dvar[d,m] = -2 dk_d^T K^-1 k*.
The first tests pin these formulas against scikit-learn's Matern kernel on the CPU; the rest (marked gpu) hold the device
against them and against its own mean / variance / covariance."""
import numpy as np
import pytest

from tests.conftest import assert_parity, relmax

SQ3, SQ5 = np.sqrt(3.0), np.sqrt(5.0)
G0 = {1.5: 3.0, 2.5: 5.0 / 3.0}


# ---------------------------------------------------------------------------------------------- numpy reference
def np_kernel(Xq, X, c, ls, nu):
    """k (M,N), c g (M,N) and u (M,N,D) of c * Matern(ls, nu)."""
    ls = np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=np.float64)), (X.shape[1],))
    diff = X[None, :, :] - Xq[:, None, :]
    r = np.sqrt(np.sum((diff / ls) ** 2, axis=-1))
    if nu == 1.5:
        t = SQ3 * r
        e = np.exp(-t)
        k, g = (1.0 + t) * e, 3.0 * e
    elif nu == 2.5:
        t = SQ5 * r
        e = np.exp(-t)
        k, g = (1.0 + t + t * t / 3.0) * e, (5.0 / 3.0) * (1.0 + t) * e
    else:
        raise ValueError(nu)
    return c * k, c * g, diff / ls ** 2


def np_gram(X, c, ls, nu):
    return np_kernel(X, X, c, ls, nu)[0]


def np_posterior(Xq, X, Y, c, ls, nu, noise=0.0, alpha=1e-10, Sigma=None):
    """mean (M,O), var (M,), J (M,O,D), Jvar (M,D), dvar (D,M) of the exact GP, K^-1 by np.linalg.solve.
    Sigma (N,N) replaces the noise diagonal (the noise-matrix model); var then carries no noise."""
    N, D = X.shape
    K = np_gram(X, c, ls, nu) + (alpha * np.eye(N) + (Sigma if Sigma is not None else noise * np.eye(N)))
    a = np.linalg.solve(K, Y)
    k, g, u = np_kernel(Xq, X, c, ls, nu)
    dk = g[:, :, None] * u                                           # (M,N,D)
    Kk = np.linalg.solve(K, k.T)                                     # (N,M)
    Kdk = np.linalg.solve(K, dk.transpose(1, 0, 2).reshape(N, -1)).reshape(N, -1, D)   # (N,M,D)
    lsv = np.broadcast_to(np.atleast_1d(np.asarray(ls, dtype=np.float64)), (D,))
    mean = k @ a
    var = c + (noise if Sigma is None else 0.0) - np.einsum("mn,nm->m", k, Kk)
    J = np.einsum("mnd,no->mod", dk, a)
    Jvar = c * G0[nu] / lsv ** 2 - np.einsum("mnd,nmd->md", dk, Kdk)
    dvar = -2.0 * np.einsum("mnd,nm->dm", dk, Kk)
    return mean, var, J, Jvar, dvar


def matern(c, ls, nu, noise):
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel
    return ConstantKernel(c) * Matern(length_scale=ls, nu=nu) + WhiteKernel(noise)


def problem(N, D, seed, O=2, M=200):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = np.stack([np.sin(3 * X @ rng.standard_normal(D)) for _ in range(O)], axis=1) + 0.01 * rng.standard_normal((N, O))
    Xq = rng.uniform(-0.1, 1.1, (M, D))
    return X, Y, Xq


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("nu", [1.5, 2.5])
@pytest.mark.parametrize("ard", [False, True])
def test_numpy_formulas_against_sklearn_matern(nu, ard):
    """d k / d x_d of the in-file formulas against central differences of sklearn's Matern.__call__, and the prior derivative
    variance c g(0) / l_d^2 against the second difference of k at tau = 0."""
    from sklearn.gaussian_process.kernels import Matern
    rng = np.random.default_rng(7)
    D, c = 3, 0.7
    ls = np.array([0.4, 0.9, 0.6]) if ard else 0.55
    X = rng.uniform(0, 1, (40, D))
    Xq = rng.uniform(0, 1, (25, D))
    sk = Matern(length_scale=ls, nu=nu)
    k, g, u = np_kernel(Xq, X, c, ls, nu)
    assert_parity(k, c * sk(Xq, X), 1e-13, "k against sklearn")
    h = 1e-6
    for d in range(D):
        e = np.zeros(D); e[d] = h
        fd = c * (sk(Xq + e, X) - sk(Xq - e, X)) / (2 * h)
        assert_parity(g * u[:, :, d], fd, 1e-7, f"dk/dx_{d}")
    lsv = np.broadcast_to(np.atleast_1d(ls), (D,))
    for d in range(D):
        tau = 1e-5 * lsv[d]
        x0 = np.zeros((1, D)); xt = x0.copy(); xt[0, d] = tau
        second = 2.0 * c * (sk(x0, x0)[0, 0] - sk(xt, x0)[0, 0]) / tau ** 2        # -k''(0) by a symmetric second difference
        assert second == pytest.approx(c * G0[nu] / lsv[d] ** 2, rel=1e-4)


def test_transportation_passes_the_flag_to_its_regressor():
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    tr = GaussianProcessTransportation(kernel_transport=matern(0.1, 0.3, 2.5, 1e-4), optimizer=None, verbose=False,
                                       matern_derivatives=True)
    assert tr.method.delta_map.matern_derivatives is True
    tr = GaussianProcessTransportation(kernel_transport=matern(0.1, 0.3, 2.5, 1e-4), optimizer=None, verbose=False)
    assert tr.method.delta_map.matern_derivatives is False


# ---------------------------------------------------------------------------------------------- GPU
def fit_gp(X, Y, c, ls, nu, noise, **kw):
    from gaussian_process_transportation_amd import GaussianProcess
    gp = GaussianProcess(kernel=matern(c, ls, nu, noise), optimizer=None, verbose=False, matern_derivatives=True, **kw)
    return gp.fit(X, Y)


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1.5, 2.5])
@pytest.mark.parametrize("D", [2, 3, 4, 5, 8, 12])
@pytest.mark.parametrize("ard", [False, True])
def test_outputs_against_numpy(nu, D, ard):
    """J, Jvar and dvar through every public entry point (each one picks a different variance kernel: Jacobian variance alone,
    fused with and without the d var cross terms) against the numpy reference, fp64."""
    X, Y, Xq = problem(300, D, seed=D)
    c, noise = 0.5, 1e-3
    ls = np.linspace(0.4, 0.9, D) if ard else 0.6
    gp = fit_gp(X, Y, c, ls, nu, noise)
    mean, var, J, Jvar, dvar = np_posterior(Xq, X, Y, c, ls, nu, noise)
    Jd, Jv = gp.derivative(Xq, return_var=True)
    assert_parity(Jd, J, 1e-8, "J (derivative)")
    assert_parity(Jv, np.repeat(Jvar[:, None, :], 2, axis=1), 1e-8, "Jvar (derivative)")
    assert_parity(gp.derivative(Xq), J, 1e-8, "J alone")
    assert_parity(gp.derivative_of_variance(Xq), dvar, 1e-8, "dvar")
    post = gp.posterior(Xq, jacobian_variance=True)
    assert_parity(post["mean"], mean, 1e-8, "mean (posterior)")
    assert_parity(post["var"], var, 1e-8, "var (posterior)")
    assert_parity(post["J"], J, 1e-8, "J (posterior)")
    assert_parity(post["Jvar"], Jvar, 1e-8, "Jvar (posterior)")
    gp.prefetch_posterior(Xq)
    m2, s2 = gp.predict(Xq, return_std=True)
    J2, V2 = gp.derivative(Xq, return_var=True)
    assert_parity(m2, mean, 1e-8, "mean (prefetched)")
    assert_parity(s2[:, 0] + np.sqrt(noise), np.sqrt(var), 1e-8, "std (prefetched)")
    assert_parity(J2, J, 1e-8, "J (prefetched)")
    assert_parity(V2[:, 0, :], Jvar, 1e-8, "Jvar (prefetched)")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1000, 3000])              # padded 1024 (<= 2560: the small-model regime) and 3072
@pytest.mark.parametrize("diag_half", ["0", "1"])
def test_work_split_coverage(N, diag_half, monkeypatch):
    """Batches that leave cut sweeps, a tail and whole rounds, at both model-size regimes; the Matern derivative launches run the
    plain kernel whatever GPT_VAR_DIAG_HALF asks (they have no HALF instantiation), RBF unchanged."""
    monkeypatch.setenv("GPT_VAR_DIAG_HALF", diag_half)
    nu, D, c, noise = 2.5, 3, 0.4, 1e-3
    ls = np.array([0.35, 0.5, 0.45])
    X, Y, _ = problem(N, D, seed=N, O=3)
    gp = fit_gp(X, Y, c, ls, nu, noise)
    rng = np.random.default_rng(N + 1)
    for M in (1, 7, 300, 20000):
        Xq = rng.uniform(-0.1, 1.1, (M, D))
        sub = np.unique(np.linspace(0, M - 1, min(M, 150)).astype(int))
        mean, var, J, Jvar, dvar = np_posterior(Xq[sub], X, Y, c, ls, nu, noise)
        post = gp.posterior(Xq, jacobian_variance=True)
        Jd, Jv = gp.derivative(Xq, return_var=True)
        dv = gp.derivative_of_variance(Xq)
        assert_parity(post["var"][sub], var, 1e-8, f"var (M={M})")
        assert_parity(post["J"][sub], J, 1e-8, f"J (M={M})")
        assert_parity(post["Jvar"][sub], Jvar, 1e-8, f"Jvar fused (M={M})")
        assert_parity(Jv[sub, 0, :], Jvar, 1e-8, f"Jvar alone (M={M})")
        assert_parity(dv[:, sub], dvar, 1e-8, f"dvar (M={M})")


def away_from(X, M, D, seed, gap):
    """M queries at least `gap` from every source point (Matern 3/2 is not twice differentiable at the sources)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < M:
        q = rng.uniform(0, 1, (4 * M, D))
        dist = np.min(np.linalg.norm(q[:, None, :] - X[None, :, :], axis=-1), axis=1)
        out.extend(q[dist > gap])
    return np.array(out[:M])


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1.5, 2.5])
def test_self_consistency_on_the_device(nu):
    """J and dvar against central differences of the device's own mean and variance; Jvar against the second difference of
    its posterior covariance, Var[(f(x+) - f(x-)) / 2h], with the noise diagonal removed."""
    D, c, noise = 3, 0.6, 1e-3
    ls = np.array([0.5, 0.4, 0.6])
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (200, D))
    Y = np.sin(4 * X[:, :1]) * np.cos(3 * X[:, 1:2])
    gp = fit_gp(X, Y, c, ls, nu, noise)
    Xq = away_from(X, 40, D, 12, 0.05)
    post = gp.posterior(Xq, jacobian_variance=True)
    dvar = gp.derivative_of_variance(Xq)
    h = 1e-5
    for d in range(D):
        e = np.zeros(D); e[d] = h
        op = gp.posterior(Xq + e)
        om = gp.posterior(Xq - e)
        fd_J = (op["mean"] - om["mean"]) / (2 * h)
        fd_v = (op["var"] - om["var"]) / (2 * h)
        assert relmax(post["J"][:, 0, d], fd_J[:, 0]) <= 1e-6, f"J_{d} vs central differences of the mean"
        assert relmax(dvar[d], fd_v) <= 1e-6, f"dvar_{d} vs central differences of the variance"
        fd_Jv = np.empty(len(Xq))
        for m in range(len(Xq)):
            _, cov = gp.predict(np.stack([Xq[m] + e, Xq[m] - e]), return_cov=True)
            cpp, cmm, cpm = cov[0, 0] - noise, cov[1, 1] - noise, cov[0, 1]
            fd_Jv[m] = (cpp + cmm - 2 * cpm) / (4 * h * h)
        assert relmax(post["Jvar"][:, d], fd_Jv) <= 1e-3, f"Jvar_{d} vs the covariance of the central difference"


@pytest.mark.gpu
@pytest.mark.parametrize("nu", [1.5, 2.5])
@pytest.mark.parametrize("D", [3, 5, 8, 12])      # 8: the fused layout of 16 columns in rows of 8 (k_var<float, 16, *, KT, 8>)
def test_fp32_model_against_fp64(nu, D):
    X, Y, Xq = problem(1000, D, seed=20 + D, M=2000)
    c, noise = 0.5, 1e-3
    ls = np.linspace(0.5, 0.8, D)
    o64 = fit_gp(X, Y, c, ls, nu, noise).posterior(Xq, jacobian_variance=True)
    gp32 = fit_gp(X, Y, c, ls, nu, noise, dtype="float32")
    o32 = gp32.posterior(Xq, jacobian_variance=True)
    assert o32["J"].dtype == np.float32
    d64 = fit_gp(X, Y, c, ls, nu, noise).derivative_of_variance(Xq)
    d32 = gp32.derivative_of_variance(Xq)
    prior = c * G0[nu] * float(np.max(1.0 / ls ** 2))
    assert np.max(np.abs(o32["J"] - o64["J"])) < 2e-4 * np.max(np.abs(o64["J"]))
    assert np.max(np.abs(o32["Jvar"] - o64["Jvar"])) < 2e-4 * prior
    assert np.max(np.abs(d32 - d64)) < 2e-4 * np.max(np.abs(d64))


@pytest.mark.gpu
def test_sharded_over_devices_equals_one_handle():
    from gaussian_process_transportation_amd.distributed import shard_range
    from gaussian_process_transportation_amd.device_group import DeviceGroup
    X, Y, _ = problem(700, 3, seed=5)
    c, noise, ls, nu = 0.5, 1e-3, np.array([0.4, 0.5, 0.6]), 1.5
    one = fit_gp(X, Y, c, ls, nu, noise)
    two = fit_gp(X, Y, c, ls, nu, noise, devices=[0, 0])
    assert isinstance(two._handle, DeviceGroup)
    M = 3001
    Xq = np.random.default_rng(6).uniform(0, 1, (M, 3))
    J2, V2 = two.derivative(Xq, return_var=True)
    d2 = two.derivative_of_variance(Xq)
    p2 = two.posterior(Xq, jacobian_variance=True)
    for r in range(2):
        a, b = shard_range(M, r, 2)
        J1, V1 = one.derivative(Xq[a:b], return_var=True)
        p1 = one.posterior(Xq[a:b], jacobian_variance=True)
        assert np.array_equal(J1, J2[a:b]) and np.array_equal(V1, V2[a:b])
        assert np.array_equal(one.derivative_of_variance(Xq[a:b]), d2[:, a:b])
        for key in ("mean", "var", "J", "Jvar"):
            assert np.array_equal(p1[key], p2[key][a:b]), key
    two._handle.close()


@pytest.mark.gpu
def test_transport_with_a_matern_kernel_against_numpy():
    """apply_transportation with a Matern 5/2 kernel_transport, velocities and orientations: the reference's assembly
    (policy_transportation.py:37-77) from the in-file J / Jvar."""
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    from gaussian_process_transportation_amd.affine_transform import AffineTransform
    from gaussian_process_transportation_amd.quaternion import quaternion_from_nonorthogonal, quaternion_multiply
    rng = np.random.default_rng(3)
    src = rng.uniform(0, 1, (250, 3))
    tgt = src @ np.array([[0.98, -0.17, 0.0], [0.17, 0.98, 0.0], [0.0, 0.0, 1.0]]) + 0.05 * np.sin(3 * src)
    traj = rng.uniform(0, 1, (400, 3))
    vel = rng.standard_normal((400, 3))
    ori = rng.standard_normal((400, 4)); ori /= np.linalg.norm(ori, axis=1, keepdims=True)
    c, ls, noise = 0.1, np.array([0.3, 0.35, 0.4]), 1e-4
    tr = GaussianProcessTransportation(kernel_transport=matern(c, ls, 2.5, noise), optimizer=None, verbose=False,
                                       matern_derivatives=True)
    tr.source_distribution, tr.target_distribution = src, tgt
    tr.training_traj, tr.training_delta, tr.training_ori = traj.copy(), vel.copy(), ori.copy()
    tr.fit_transportation()
    tr.apply_transportation()
    aff = AffineTransform(verbose=False).fit(src, tgt)
    src_al = aff.predict(src)
    delta = tgt - src_al
    rot = aff.predict(traj)
    mean, var, J, Jvar, _ = np_posterior(rot, src_al, delta, c, ls, 2.5, noise)
    Jg = aff.derivative(traj)
    J_phi = Jg + J @ Jg
    v_rot = Jg @ vel[:, :, None]
    assert_parity(tr.training_traj, rot + mean, 1e-8, "transported positions")
    assert_parity(tr.training_delta, (J_phi @ vel[:, :, None])[:, :, 0], 1e-8, "transported velocities")
    Sigma = np.repeat(Jvar[:, None, :], 3, axis=1)
    assert_parity(tr.var_vel_transported, (Sigma @ v_rot ** 2)[:, :, 0], 1e-8, "var_vel_transported")
    # orientations: J_Phi at the UN-rotated positions (policy_transportation.py:62)
    J_raw = np_posterior(traj, src_al, delta, c, ls, 2.5, noise)[2]
    J_phi_raw = Jg + J_raw @ Jg
    assert_parity(tr.training_ori, quaternion_multiply(quaternion_from_nonorthogonal(J_phi_raw), ori), 1e-7, "orientations")


@pytest.mark.gpu
@pytest.mark.parametrize("nu,code", [(1.5, 2), (2.5, 3)])
def test_noise_matrix_model_against_numpy(nu, code):
    from gaussian_process_transportation_amd import _lib
    rng = np.random.default_rng(9)
    N, D, c = 400, 3, 0.3
    ls = np.array([0.3, 0.4, 0.5])
    X = rng.uniform(0, 1, (N, D))
    Y = np.sin(3 * X.sum(1, keepdims=True))
    A = rng.standard_normal((N, N))
    Sigma = A @ A.T / N * 1e-3 + 1e-4 * np.eye(N)
    Xq = rng.uniform(0, 1, (500, D))
    h = _lib.Handle(0)
    h.fit_noise_matrix(X, Y, ls, c, Sigma, 1e-10, kernel_type=code)
    with pytest.raises(ValueError, match="gpt_set_matern_derivatives"):       # C ABI default: refused, as before
        h.predict_all(Xq, J=True)
    h.set_matern_derivatives(True)
    out = h.predict_all(Xq, mean=True, var=True, J=True, Jvar=True)
    dv = h.predict_all(Xq, dvar=True)["dvar"]
    h.close()
    mean, var, J, Jvar, dvar = np_posterior(Xq, X, Y, c, ls, nu, alpha=1e-10, Sigma=Sigma)
    assert_parity(out["mean"], mean, 1e-8, "mean")
    assert_parity(out["var"], var, 1e-8, "var")
    assert_parity(out["J"], J, 1e-8, "J")
    assert_parity(out["Jvar"], Jvar, 1e-8, "Jvar")
    assert_parity(dv, dvar, 1e-8, "dvar")


@pytest.mark.gpu
def test_refusals_that_remain():
    from gaussian_process_transportation_amd import GaussianProcess, _lib
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    X, Y, Xq = problem(100, 3, seed=1, M=10)
    # Matern 1/2: not differentiable at the sources, refused with or without the flag
    m12 = fit_gp(X, Y, 0.5, 0.4, 0.5, 1e-3)
    for call in (lambda: m12.derivative(Xq), lambda: m12.derivative_of_variance(Xq), lambda: m12.posterior(Xq),
                 lambda: m12.prefetch_posterior(Xq)):
        with pytest.raises(NotImplementedError, match="nu=0.5"):
            call()
    assert m12.predict(Xq).shape == (10, 2)
    # without the flag, Matern 3/2 and 5/2 keep the refusal, which now names the flag
    off = GaussianProcess(kernel=matern(0.5, 0.4, 2.5, 1e-3), optimizer=None, verbose=False).fit(X, Y)
    with pytest.raises(NotImplementedError, match="matern_derivatives"):
        off.derivative(Xq)
    # the C ABI on a Matern 1/2 handle
    h = _lib.Handle(0)
    h.set_matern_derivatives(True)
    h.fit(X, Y, [0.4], 0.5, 1e-3, 1e-10, kernel_type=1)
    for flags in (dict(J=True), dict(Jvar=True), dict(dvar=True), dict(mean=True, J=True)):
        with pytest.raises(ValueError, match="Matern 1/2"):             # GPT_E_ARG (_lib.check)
            h.predict_all(Xq, **flags)
    assert h.predict_all(Xq, mean=True, var=True)["var"].shape == (10,)
    h.close()
    # RBF models: the flag changes nothing
    kern = ConstantKernel(0.5) * RBF([0.4]) + WhiteKernel(1e-3)
    a = GaussianProcess(kernel=kern, optimizer=None, verbose=False).fit(X, Y)
    b = GaussianProcess(kernel=kern, optimizer=None, verbose=False, matern_derivatives=True).fit(X, Y)
    for x, y in zip(a.derivative(Xq, return_var=True), b.derivative(Xq, return_var=True)):
        assert np.array_equal(x, y)
    assert np.array_equal(a.derivative_of_variance(Xq), b.derivative_of_variance(Xq))
