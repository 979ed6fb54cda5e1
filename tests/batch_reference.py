"""Extended-precision (np.longdouble, 64-bit mantissa) statement of ONE small exact GP as the gpt_batch_* entry points define
it (include/gpt_hip.h; scikit-learn's GaussianProcessRegressor with the kernel c * k(r) + WhiteKernel(noise) and alpha = jitter).
Test helper only: plain numpy loops, no LAPACK (numpy's longdouble matmul is a C loop), nothing from the package under test.
tests/test_batch_precision.py pins it to 40-digit mpmath and uses it as the yardstick the fp64 kernels are held to.

    K        = c k(X, X); the diagonal is (c + noise) + jitter (k is never evaluated at r = 0 there; coincident rows off the
               diagonal do give k = c)
    L, alpha = cholesky(K), K^-1 Y                         lml = -1/2 sum Y.alpha - O sum log L_ii - O n/2 log 2 pi
    grad     = 1/2 tr((alpha alpha^T - O K^-1) dK/dtheta), theta = log [c, l (1 or D of them), noise]; the jitter is in no
               gradient, the Matern 1/2 length-scale term is 0 where r = 0, the isotropic gradient is one summed entry
    mean (M, O) = k* alpha        var (M,) = max(c + noise - |L^-1 k*|^2, 0)     (the noise is part of var)
    RBF only:  J (M, O, D) = dk*_d alpha, dk*_d = k* (X_d - x_d) / l_d^2;  Jvar (M, D) = c / l_d^2 - |L^-1 dk*_d|^2;
               dvar (M, D) = -2 (L^-1 dk*_d).(L^-1 k*)
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, (
    f"tests/batch_reference.py needs an extended-precision np.longdouble (x87 80-bit: eps 1.08e-19); this platform's has eps "
    f"{np.finfo(LD).eps:.3g}, which would make the reference no better than the fp64 kernels it judges")

KINDS = ("rbf", "matern12", "matern32", "matern52")        # in the order of the kernel_type codes 0 .. 3
PI = 4 * np.arctan(LD(1))


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)      # fp64 inputs are exact in longdouble


def _shape(kind, r):
    """k(r) and g(r) of dk/dlog l_d = g(r) u_d^2, u = (x - x') / l (sklearn kernels.py RBF 1553-1580, Matern 1717-1778)."""
    if kind == "rbf":
        k = np.exp(-r * r / 2)
        return k, k
    if kind == "matern12":
        k = np.exp(-r)
        pos = r > 0
        g = np.zeros_like(k)
        g[pos] = k[pos] / r[pos]
        return k, g
    if kind == "matern32":
        t = np.sqrt(LD(3)) * r
        e = np.exp(-t)
        return (1 + t) * e, 3 * e
    if kind == "matern52":
        t = np.sqrt(LD(5)) * r
        e = np.exp(-t)
        return (1 + t + t * t / 3) * e, LD(5) / 3 * (1 + t) * e
    raise ValueError(kind)


def _scaled_diff(A, B, ls):
    """u[i, j, d] = (A[i, d] - B[j, d]) / l_d"""
    return (A[:, None, :] - B[None, :, :]) / ls


def cholesky(K):
    """Lower factor, a column at a time.  Raises np.linalg.LinAlgError on a pivot that is not positive."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        d = K[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is {d}")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_inverse(L):
    """W = L^-1 by forward substitution on the identity, a row at a time."""
    n = L.shape[0]
    W = np.zeros_like(L)
    for i in range(n):
        e = np.zeros(n, dtype=LD)
        e[i] = 1
        W[i] = (e - L[i, :i] @ W[:i]) / L[i, i]
    return W


def gp(kind, X, Y, c, ls, noise, jitter, Xq=None):
    """Every quantity of one model, as longdouble arrays in the layouts of _lib.batch_fit / batch_lml_objective / batch_predict.
    ls: 1 entry (isotropic: grad has 3 entries) or D entries (ARD: 2 + D).  Xq (M, D) adds the posterior at the queries."""
    X, Y = _ld(X), _ld(Y)
    n, D = X.shape
    O = Y.shape[1]
    ls = _ld(ls).reshape(-1)
    n_ls = ls.size
    assert n_ls in (1, D)
    lsv = np.broadcast_to(ls, (D,))
    c, noise, jitter = LD(c), LD(noise), LD(jitter)

    U2 = _scaled_diff(X, X, lsv) ** 2                       # (n, n, D)
    r = np.sqrt(U2.sum(-1))
    k, g = _shape(kind, r)
    eye = np.eye(n, dtype=bool)
    R = np.where(eye, LD(1), k)                             # dK / dlog c = c R; the diagonal of k itself is never used
    K = c * R
    K[eye] = (c + noise) + jitter
    L = cholesky(K)
    W = lower_inverse(L)
    alpha = W.T @ (W @ Y)
    out = {"K": K, "L": L, "alpha": alpha,
           "lml": -(Y * alpha).sum() / 2 - O * np.log(np.diag(L)).sum() - O * LD(n) / 2 * np.log(2 * PI)}
    inner = alpha @ alpha.T - O * (W.T @ W)
    G = np.where(eye, LD(0), c * g)
    grad = np.empty(2 + n_ls, dtype=LD)
    grad[0] = (inner * (c * R)).sum() / 2
    if n_ls == 1:
        grad[1] = (inner * G * U2.sum(-1)).sum() / 2
    else:
        for d in range(D):
            grad[1 + d] = (inner * G * U2[:, :, d]).sum() / 2
    grad[1 + n_ls] = noise * np.trace(inner) / 2
    out["grad"] = grad
    if Xq is None:
        return out

    Xq = _ld(Xq)
    Uq = _scaled_diff(Xq, X, lsv)                           # (M, n, D): (x_m - X_k) / l
    Ks = c * _shape(kind, np.sqrt((Uq ** 2).sum(-1)))[0]    # (M, n)
    V = W @ Ks.T                                            # (n, M)
    out["mean"] = Ks @ alpha
    out["var"] = np.maximum((c + noise) - (V * V).sum(0), LD(0))
    if kind == "rbf":
        M = Xq.shape[0]
        J, Jvar, dvar = np.empty((M, O, D), dtype=LD), np.empty((M, D), dtype=LD), np.empty((M, D), dtype=LD)
        for d in range(D):
            dk = Ks * (-Uq[:, :, d] / lsv[d])               # k* (X_d - x_d) / l_d^2
            Vd = W @ dk.T
            J[:, :, d] = dk @ alpha
            Jvar[:, d] = c / (lsv[d] * lsv[d]) - (Vd * Vd).sum(0)
            dvar[:, d] = -2 * (Vd * V).sum(0)
        out.update(J=J, Jvar=Jvar, dvar=dvar)
    return out


def relmax(a, b):
    """max |a - b| / max |b|, as tests/conftest.py's relmax, without rounding the reference b to fp64 first."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else LD(1)))
