"""Pathwise conditioning restated in numpy, for tests/test_pathwise_cpu.py and tests/test_rollout_pathwise.py.

A function drawn by gaussian_process_transportation_amd/posterior_functions.py is
    F(x) = prior(x) + k(x, X) (K + s^2 I)^-1 (Y - prior(X) - s eps),      prior(x) = phi(x) . w,  w ~ N(0, I),
with phi(x) = sqrt(c / J) [cos(omega_j . x), sin(omega_j . x)] (2 J features).  With A = K* (K + s^2 I)^-1 its covariance at the
queries is, in closed form,
    B B^T + s^2 A A^T,   B = Phi* - A Phi,
which would be the exact latent posterior covariance K** - A K*^T if Phi Phi^T were the prior covariance; what is left is the
error of the features, of order 1 / sqrt(J).  Nothing here reads the device; the kernels come from tests/posterior_restatement.py.

function_values(): one evaluation of drawn functions in longdouble with the sums of the absolute terms, the reference and the
rounding floor of the device's one-step values."""
import numpy as np

from tests import posterior_restatement as PR

LD = np.longdouble
KIND_CODE = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3}


def kernel_matrix(A, B, c, ls, kind, ty=np.float64):
    """c k(a, b) without noise, (len A, len B), in the arithmetic of `ty`."""
    lsv = PR._full_ls(ls, A.shape[1]).astype(ty)
    a2, _ = PR._sq(A.astype(ty) / lsv, B.astype(ty) / lsv)
    return ty(c) * PR.shapes(a2, kind, ty)[0]


def features(X, omega, c):
    """Phi (N, 2 J): sqrt(c / J) [cos(X omega^T), sin(X omega^T)], so that prior_at(X, omega, amp)[s, :, o] = Phi @ w with
    w = [amp[s, :, 0, o], amp[s, :, 1, o]] / sqrt(c / J)."""
    theta = X @ omega.T
    return np.sqrt(c / omega.shape[0]) * np.concatenate([np.cos(theta), np.sin(theta)], axis=1)


def _solve_weights(X, Xq, c, ls, noise, kind):
    """A = K* (K + noise I)^-1 (M,N) with scipy's Cholesky solve, and K, K*, K** in fp64."""
    from scipy.linalg import cho_factor, cho_solve
    K = kernel_matrix(X, X, c, ls, kind)
    Ks = kernel_matrix(Xq, X, c, ls, kind)
    Kss = kernel_matrix(Xq, Xq, c, ls, kind)
    A = cho_solve(cho_factor(K + noise * np.eye(len(X)), lower=True), Ks.T).T
    return A, K, Ks, Kss


def posterior_cov(X, Xq, c, ls, noise, kind):
    """The exact latent posterior covariance K** - A K*^T in fp64."""
    A, _, Ks, Kss = _solve_weights(X, Xq, c, ls, noise, kind)
    return Kss - A @ Ks.T


def posterior_cov_longdouble(X, Xq, c, ls, noise, kind):
    """The same in 80-bit arithmetic throughout: K** - V^T V, V = L^-1 K*^T."""
    K = kernel_matrix(X, X, c, ls, kind, LD)
    K[np.diag_indices_from(K)] += LD(noise)
    L = PR.cholesky_columns(K)
    V = PR.forward_substitution(L, np.ascontiguousarray(kernel_matrix(Xq, X, c, ls, kind, LD).T))
    return kernel_matrix(Xq, Xq, c, ls, kind, LD) - V.T @ V


def construction_cov(X, Xq, c, ls, noise, kind, omega=None):
    """B B^T + noise A A^T of the construction with the frequencies omega (J,D); omega None: with Phi Phi^T replaced by the exact
    prior covariance, B B^T = K** - A K*^T - K* A^T + A K A^T."""
    A, K, Ks, Kss = _solve_weights(X, Xq, c, ls, noise, kind)
    if omega is None:
        BBt = Kss - A @ Ks.T - Ks @ A.T + A @ K @ A.T
    else:
        B = features(Xq, omega, c) - A @ features(X, omega, c)
        BBt = B @ B.T
    return BBt + noise * (A @ A.T)


def function_values(X, c, ls, kind, weights, omega, amp, func, x, ty=LD):
    """F_s(x_p), s = func[p], at the points x (P,D) in the arithmetic of `ty` (longdouble: the reference; float64: its twin, whose
    distance from the reference is the error of the oracle): value (P,O) and floor (P,O) = the sum of the absolute terms, the
    kernel terms |k(x, X_n) V[n, o]| as they are and a feature term |a cos| + |b sin| weighted by 1 + |theta_j| (theta_j is a
    rounded fp64 number of that size before the sine and cosine are taken)."""
    lsv = PR._full_ls(ls, X.shape[1]).astype(ty)
    xl, Xl = x.astype(ty), X.astype(ty)
    a2, _ = PR._sq(xl / lsv, Xl / lsv)                           # (P, N)
    k = ty(c) * PR.shapes(a2, kind, ty)[0]
    V = weights.astype(ty)[func]                                 # (P, N, O)
    value = np.einsum("pn,pno->po", k, V)
    floor = np.einsum("pn,pno->po", np.abs(k), np.abs(V))
    if omega.shape[0]:
        theta = xl @ omega.astype(ty).T                          # (P, J)
        ab = amp.astype(ty)[func]                                # (P, J, 2, O)
        cs, sn = np.cos(theta), np.sin(theta)
        value = value + np.einsum("pj,pjo->po", cs, ab[:, :, 0]) + np.einsum("pj,pjo->po", sn, ab[:, :, 1])
        wt = ty(1) + np.abs(theta)
        floor = floor + np.einsum("pj,pjo->po", wt * np.abs(cs), np.abs(ab[:, :, 0])) + np.einsum("pj,pjo->po", wt * np.abs(sn), np.abs(ab[:, :, 1]))
    return value, floor
