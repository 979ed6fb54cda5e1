"""Extended-precision (np.longdouble) statement of gpt_batch_fold_scan (include/gpt_hip.h) for ONE model.  Test helper only: plain numpy, nothing from
the package under test.  The factorisation is tests/batch_reference.py's (pinned to 40-digit mpmath by test_batch_precision.py);
tests/test_fold_scan_cpu.py pins what is added here to mpmath, to scikit-learn's predict and to a central finite difference.

    alpha = K(X)^-1 Y                       psi(x) = k(x, X) alpha        J[o][d] = d psi_o / d x_d
    det   = det(I + J)                      z = x + psi(x)
    surrogate: Xs = fl64(X + Y), beta = K(Xs)^-1 (-Y), psi_inv(z) = k(z, Xs) beta, err = |psi(x) + psi_inv(z)|_2
    per model: min det, the first index attaining it, the count of det <= 0, the sum and the maximum of err

`scan_fp64` is the same computation in plain fp64 (LAPACK Cholesky): its distance from `scan` is the e_oracle of the tolerance
rule of tests/test_batch_precision.py, a measure of what fp64 can resolve on the case at hand."""
import numpy as np

from tests import batch_reference as br

LD = br.LD
OK, NOT_PD = 0, -2                                        # GPT_OK, GPT_E_NOT_PD


def _mean_jac(X, alpha, c, lsv, Xq):
    """psi (M, D) and J (M, D, D) at Xq, in the dtype of the arguments."""
    U = (Xq[:, None, :] - X[None, :, :]) / lsv            # (M, n, D): (x - X_k) / l
    Ks = c * np.exp(-(U * U).sum(-1) / 2)                 # (M, n)
    J = np.empty((Xq.shape[0], alpha.shape[1], X.shape[1]), dtype=Ks.dtype)
    for d in range(X.shape[1]):
        J[:, :, d] = (Ks * (-U[:, :, d] / lsv[d])) @ alpha   # k* (X_d - x_d) / l_d^2
    return Ks @ alpha, J


def det_i_plus(J):
    """det(I + J) in closed form, D = 1, 2, 3."""
    A = J + np.eye(J.shape[-1], dtype=J.dtype)
    D = A.shape[-1]
    if D == 1:
        return A[:, 0, 0]
    if D == 2:
        return A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    return (A[:, 0, 0] * (A[:, 1, 1] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 1]) - A[:, 0, 1] * (A[:, 1, 0] * A[:, 2, 2] - A[:, 1, 2] * A[:, 2, 0])
            + A[:, 0, 2] * (A[:, 1, 0] * A[:, 2, 1] - A[:, 1, 1] * A[:, 2, 0]))


def _alpha(X, Y, c, ls, noise, jitter, dtype):
    """K(X)^-1 Y, or None where K is not positive definite."""
    try:
        if dtype is LD:
            return br.gp("rbf", X, Y, c, ls, noise, jitter)["alpha"]
        import scipy.linalg
        lsv = np.broadcast_to(np.asarray(ls, dtype=np.float64).reshape(-1), (X.shape[1],))
        U = (X[:, None, :] - X[None, :, :]) / lsv
        K = c * np.exp(-(U * U).sum(-1) / 2)
        K[np.diag_indices_from(K)] = (c + noise) + jitter
        return scipy.linalg.cho_solve((np.linalg.cholesky(K), True), Y)
    except np.linalg.LinAlgError:
        return None


def scan(X, Y, c, ls, noise, jitter, Xq, surrogate=True, dtype=LD):
    """Every output of gpt_batch_fold_scan for one model: a dict with status, surrogate_status, the per-query arrays psi, J, det,
    z, err and the reductions min_det, argmin, n_fold, err_sum, err_max (None for what the call leaves untouched)."""
    X, Y, Xq = (np.asarray(a, dtype=np.float64) for a in (X, Y, Xq))
    D = X.shape[1]
    out = dict(status=OK, surrogate_status=OK if surrogate else None, err=None, err_sum=None, err_max=None)
    alpha = _alpha(X, Y, c, ls, noise, jitter, dtype)
    if alpha is None:
        return dict(status=NOT_PD)
    lsv = np.broadcast_to(np.asarray(ls, dtype=np.float64).reshape(-1), (D,)).astype(dtype)
    cc = dtype(c)
    xq = Xq.astype(dtype)
    psi, J = _mean_jac(X.astype(dtype), alpha, cc, lsv, xq)
    det = det_i_plus(J)
    z = xq + psi
    out.update(psi=psi, J=J, det=det, z=z)
    M = Xq.shape[0]
    out.update(min_det=det.min() if M else dtype(np.inf), argmin=int(np.argmin(det)) if M else -1, n_fold=int((det <= 0).sum()))
    if surrogate:
        Xs = X + Y                                        # rounded to fp64: the reference's target_distribution
        beta = _alpha(Xs, -Y, c, ls, noise, jitter, dtype)
        if beta is None:
            out["surrogate_status"] = NOT_PD
            return out
        psi_inv, _ = _mean_jac(Xs.astype(dtype), beta, cc, lsv, z)
        err = np.sqrt(((psi + psi_inv) ** 2).sum(-1))
        out.update(err=err, err_sum=err.sum() if M else dtype(0), err_max=err.max() if M else dtype(0))
    return out


def scan_fp64(*args, **kw):
    return scan(*args, dtype=np.float64, **kw)
