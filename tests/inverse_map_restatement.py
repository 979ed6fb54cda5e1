"""numpy restatement of the device's inverse of the displacement map (csrc/gpt_inverse.hip, gpt_inverse_map of
include/gpt_hip.h): the same damped Newton iteration, over the CPU oracle's predict / derivative.  Not a test; imported by
tests/test_inverse_map.py, examples and tools.

Per query, fp64:
    z <- z0 (y when none);  r <- z + mu(z) - y;  A <- I + J(z);  rho <- |r|;  tol <- rtol (1 + |y|);  t <- 1;  passes <- 1
    repeat:  rho <= tol -> CONVERGED;  passes == max_passes -> MAX_PASSES;  |det A| <= 2^-40 |A|_F^D -> SINGULAR
             z' <- z - t A^-1 r;  r', A' at z';  passes += 1;  rho' <- |r'|
             rho' < rho -> accept, t <- min(1, 2t);  else t <- t / 2, t < 2^-20 -> STALLED
All queries advance together here (one model evaluation per pass over those still running); each follows the iteration
above on its own."""
import numpy as np

from oracle.gp_oracle import GaussianProcessOracle, kernel_cross

CONVERGED, MAX_PASSES, SINGULAR, STALLED = 0, 1, 2, 3


class RbfModel:
    """mu, J and sum_n |k alpha_n| of a fitted GaussianProcessOracle (RBF)."""

    def __init__(self, gp: GaussianProcessOracle):
        self.gp = gp

    def mean_jac(self, z):
        return self.gp.predict(z).reshape(len(z), -1), self.gp.derivative(z)

    def abs_sum(self, z):
        k = kernel_cross(z, self.gp.X, self.gp.constant_value, self.gp._ls())
        return np.abs(k) @ np.abs(self.gp.alpha_.reshape(len(self.gp.X), -1))


class MaternModel:
    """The same for c * Matern(ls, nu) + noise, nu = 1.5 / 2.5, with the g(r) derivative coefficient as
    tests/test_matern_derivatives.py restates it."""

    def __init__(self, X, Y, c, ls, nu, noise, alpha=1e-10):
        from tests.test_matern_derivatives import np_gram
        self.X, self.c, self.ls, self.nu = X, c, ls, nu
        K = np_gram(X, c, ls, nu) + (noise + alpha) * np.eye(len(X))
        self.a = np.linalg.solve(K, Y)

    def mean_jac(self, z):
        from tests.test_matern_derivatives import np_kernel
        k, g, u = np_kernel(z, self.X, self.c, self.ls, self.nu)
        return k @ self.a, np.einsum("mnd,no->mod", g[:, :, None] * u, self.a)

    def abs_sum(self, z):
        from tests.test_matern_derivatives import np_kernel
        return np.abs(np_kernel(z, self.X, self.c, self.ls, self.nu)[0]) @ np.abs(self.a)


def residual_and_jacobian(model, z, y):
    mu, J = model.mean_jac(z)
    return z + mu - y, np.eye(z.shape[1])[None] + J


def inverse_map(model, y, z0=None, rtol=1e-10, max_passes=64):
    """(z (M,D), info) with info = {status, passes, residual, det} as the device returns them."""
    y = np.asarray(y, dtype=np.float64)
    M, D = y.shape
    z = y.copy() if z0 is None else np.array(z0, dtype=np.float64)
    r, A = residual_and_jacobian(model, z, y)
    rho = np.linalg.norm(r, axis=1)
    tol = rtol * (1.0 + np.linalg.norm(y, axis=1))
    t = np.ones(M)
    passes = np.ones(M, dtype=np.int32)
    status = np.full(M, -1, dtype=np.int32)
    while True:
        run = status < 0
        status[run & (rho <= tol)] = CONVERGED
        run = status < 0
        status[run & (passes == max_passes)] = MAX_PASSES
        run = status < 0
        det = np.linalg.det(A)
        fro = np.sqrt(np.sum(A * A, axis=(1, 2)))
        status[run & (np.abs(det) <= 2.0 ** -40 * fro ** D)] = SINGULAR
        idx = np.flatnonzero(status < 0)
        if idx.size == 0:
            break
        s = np.linalg.solve(A[idx], r[idx][:, :, None])[:, :, 0]
        zn = z[idx] - t[idx, None] * s
        rn, An = residual_and_jacobian(model, zn, y[idx])
        passes[idx] += 1
        rhon = np.linalg.norm(rn, axis=1)
        ok = rhon < rho[idx]                       # (false for NaN)
        acc, rej = idx[ok], idx[~ok]
        z[acc], r[acc], A[acc], rho[acc] = zn[ok], rn[ok], An[ok], rhon[ok]
        t[acc] = np.minimum(1.0, 2.0 * t[acc])
        t[rej] *= 0.5
        status[rej[t[rej] < 2.0 ** -20]] = STALLED
    return z, {"status": status, "passes": passes, "residual": rho, "det": np.linalg.det(A)}


def error_bound(model, z, y, rtol):
    """What separates a CONVERGED z from the exact preimage, to first order: |A^-1|_2 times the residual the stopping rule
    allows plus the rounding floor of the device's sums, 64 eps S with S the norm over the outputs of sum_n |k(z, X_n) alpha_n|
    (a lane adds at most ceil(N / 64) <= 40 terms at the sizes tested, the butterfly 6 more, each term carries the table
    exp's 1.6 eps).  Returns (bound (M,), floor (M,)); the tests allow twice the bound."""
    _, A = residual_and_jacobian(model, z, y)
    inv_norm = 1.0 / np.linalg.svd(A, compute_uv=False)[:, -1]
    floor = 64.0 * np.finfo(np.float64).eps * np.linalg.norm(model.abs_sum(z), axis=1)
    return (rtol * (1.0 + np.linalg.norm(y, axis=1)) + floor) * inv_norm, floor
