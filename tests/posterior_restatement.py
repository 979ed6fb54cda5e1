"""Two restatements of the exact-GP main path (fit, the five outputs of predict_all, the LML and its gradient) for the tests
that hold the library elementwise.  Helper module: no tests here.

posterior_longdouble   plain numpy in 80-bit arithmetic, the formulas of oracle/gp_oracle.py and of np_posterior in
                       tests/test_matern_derivatives.py (analytic Matern derivatives with g(r), prior c g(0) / l_d^2), the
                       column-loop Cholesky and forward substitution of tests/test_covariance_and_handle_reuse.py.
posterior_float64      the library's own algebra in fp64 numpy: sources stored as X (1 / l), coordinates scaled before they are
                       subtracted, h from squared differences of the scaled coordinates, k* = pre(t) exp(ln c - t), explicit
                       W = L^-1, V = W k*, var = c + noise - |V|^2, K^-1 = W^T W in the gradient.
reference              both on the same inputs, and from them the elementwise tolerance of every output.

The tolerance rule.  |library - longdouble| <= 16 max(e_ref, floor) for every element, where
    floor = 64 x 2^-52 x scale + underflow,     e_ref = scale x max over the array of |float64 - longdouble| / scale.
`scale` is the natural magnitude of that element (SCALES below); e_ref is what fp64 costs this operation on these inputs, as the
fp64 restatement measures it, in units of the element's scale: for var and Jvar (one scale for the whole array) that is the
plain largest deviation, for mean, J and dvar it follows the element down as k* fades, so that a mean of 1e-200 is held to
1e-200 x (a few hundred ulps) and not to the error of the largest mean.  16 is the margin for another summation order (MFMA
blocks, wave reductions, a blocked inverse) and 64 ulps the floor, both as in test_covariance_and_handle_reuse.py; neither comes
from a run of the library.  `underflow` is the one term the rule needs where k* is subnormal: a double below 2.2e-308 is
rounded to a multiple of 2^-1074, not to 2^-53 of itself, so a sum of k*_n alpha_n carries up to 2^-1074 pre_n (|alpha_n| + 1)
per term whoever computes it in doubles (pre: the Matern polynomial that multiplies the exponential; |alpha_n| for the rounding
of the exponential, 1 for that of its product with alpha_n, which is subnormal too where |alpha_n| < 1; in J both are multiplied
by |u_nd| afterwards), and the result itself is a multiple of 2^-1074.  All of it is 1e-320 times the coefficients and beside
the point wherever k* is a normal number."""
import numpy as np

from tests.test_covariance_and_handle_reuse import cholesky_columns, forward_substitution     # column loop, row loop

LD = np.longdouble
EPS = 2.0 ** -52
TINY = 2.0 ** -1074                                        # spacing of the subnormal doubles
RS2, S2 = 0.70710678118654752440, 1.41421356237309504880
MARGIN, FLOOR_ULPS = 16.0, 64.0
KINDS = ("rbf", "matern12", "matern32", "matern52")        # index = kernel_type of the C ABI
G0 = {"rbf": 1.0, "matern32": 3.0, "matern52": 5.0 / 3.0}   # g(0): prior derivative variance c g(0) / l_d^2
OUTPUTS = ("mean", "var", "J", "Jvar", "dvar")
SCALES = {"mean": "sum_n (1 + h_n) |k*_n alpha_n|", "J": "sum_n (1 + h_n) |g_n alpha_n u_nd|", "var": "c + noise",
          "Jvar": "c g(0) / l_d^2", "dvar": "2 |V| |V_d|", "grad": "1/2 sum_ij |inner_ij dK_ij / dtheta_p|",
          "lml": "1/2 |y^T alpha| + sum |log L_ii| + 1/2 O N log 2 pi"}


def longdouble_is_extended():
    return np.finfo(LD).eps <= 1e-18


# --------------------------------------------------------------------------- linear algebra in the operands' own precision
def backward_substitution(L, B):
    """L^T \\ B."""
    return forward_substitution(L.T[::-1, ::-1], B[::-1])[::-1]


# --------------------------------------------------------------------------- kernel shapes
def shapes(a2, kind, ty, lnc=None):
    """From a2 = r^2 (any shape): k / c, g / c (None for Matern 1/2), pre_k, pre_g (the polynomials in front of the
    exponential) and the exponent's argument t (k = pre_k exp(-t)).  With lnc the exponential is exp(lnc - t), as the
    prediction kernels take it, and the first two results carry the factor c."""
    a2 = np.asarray(a2, dtype=ty)
    one = ty(1)
    if kind == "rbf":
        t = a2 / ty(2)
        pre_k = pre_g = np.ones_like(a2)
    else:
        r = np.sqrt(a2)
        if kind == "matern12":
            t, pre_k, pre_g = r, np.ones_like(a2), None
        elif kind == "matern32":
            t = np.sqrt(ty(3)) * r
            pre_k, pre_g = one + t, np.full_like(a2, 3)
        elif kind == "matern52":
            t = np.sqrt(ty(5)) * r
            pre_k, pre_g = one + t + t * t / ty(3), ty(5) / ty(3) * (one + t)
        else:
            raise ValueError(kind)
    with np.errstate(under="ignore"):
        e = np.exp(-t) if lnc is None else np.exp(ty(lnc) - t)
        k = pre_k * e
        g = None if pre_g is None else pre_g * e
    return k, g, pre_k, pre_g, t


def lml_shape(a2, k, g, kind):
    """G of dK / dlog l_d = c G D_d, D_d = (x_d - x'_d)^2 / l_d^2: k (RBF), k / r (Matern 1/2, 0 at r = 0), g (3/2, 5/2)."""
    if kind == "rbf":
        return k
    if kind == "matern12":
        r = np.sqrt(a2)
        return np.divide(k, r, out=np.zeros_like(k), where=r != 0)
    return g


def _sq(A, B):
    """(|a - b|^2 (len A, len B), the per-coordinate differences b_d - a_d as a list of (len A, len B))."""
    diffs = [B[:, d][None, :] - A[:, d][:, None] for d in range(A.shape[1])]
    a2 = np.zeros((A.shape[0], B.shape[0]), dtype=A.dtype)
    for df in diffs:
        a2 += df * df
    return a2, diffs


def _full_ls(ls, D):
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    return np.full(D, ls[0]) if ls.size == 1 else ls


# --------------------------------------------------------------------------- the longdouble restatement
def posterior_longdouble(X, Y, c, ls, noise, jitter, kind, Xq=None, derivatives=True, gradient=True):
    """Everything in 80-bit arithmetic.  Returns a dict: L, alpha, lml, and with `gradient` grad_ard (2 + D) / grad_iso (3) in
    theta = log(c, l.., noise) with their scales; with queries mean (M,O), var (M,), kstar (M,N) and, with `derivatives`
    (never for Matern 1/2), J (M,O,D), Jvar (M,D), dvar (D,M); scale_<output> and under_<output> for the tolerance rule."""
    N, D = X.shape
    O = Y.shape[1]
    c_, noise_ = LD(c), LD(noise)
    lsv = _full_ls(ls, D).astype(LD)
    Xl, Yl = X.astype(LD), Y.astype(LD)
    Xs = Xl / lsv
    a2, diffs = _sq(Xs, Xs)
    k, g, _, _, _ = shapes(a2, kind, LD)
    K = c_ * k
    K[np.diag_indices_from(K)] += noise_ + LD(jitter)
    L = cholesky_columns(K)
    alpha = backward_substitution(L, forward_substitution(L, Yl))
    logdiag = np.log(np.diag(L))
    ya = np.einsum("no,no->o", Yl, alpha)
    half_log_2pi = LD(N) / LD(2) * np.log(LD(8) * np.arctan(LD(1)))
    out = {"K": K, "L": L, "alpha": alpha, "lml": (-ya / LD(2)).sum() - O * logdiag.sum() - O * half_log_2pi,
           "scale_lml": np.abs(ya).sum() / LD(2) + O * np.abs(logdiag).sum() + O * half_log_2pi}
    if gradient:
        W = forward_substitution(L, np.eye(N, dtype=LD))
        inner = alpha @ alpha.T - O * (W.T @ W)
        Gc = c_ * lml_shape(a2, k, g, kind)
        terms = [inner * (c_ * k)] + [inner * Gc * (df * df) for df in diffs] + [np.diag(np.diag(inner) * noise_)]
        sums = np.array([t.sum() for t in terms], dtype=LD) / LD(2)
        mags = np.array([np.abs(t).sum() for t in terms], dtype=LD) / LD(2)
        out["grad_ard"], out["scale_grad_ard"] = sums, mags
        iso = np.abs(sum(terms[1:1 + D])).sum() / LD(2)
        out["grad_iso"] = np.array([sums[0], sums[1:1 + D].sum(), sums[-1]], dtype=LD)
        out["scale_grad_iso"] = np.array([mags[0], iso, mags[-1]], dtype=LD)
    if Xq is None:
        return out
    M = Xq.shape[0]
    Ql = Xq.astype(LD)
    a2q, _ = _sq(Ql / lsv, Xs)                               # (M, N)
    kq, gq, pre_k, pre_g, tq = shapes(a2q, kind, LD)
    out["arg_min"] = tq.min(1).astype(np.float64)            # smallest argument of the exponential behind each query
    ks = c_ * kq
    amp = LD(1) + a2q / LD(2)                                # 1 + h_n
    A = np.abs(alpha)
    V = forward_substitution(L, np.ascontiguousarray(ks.T))  # (N, M)
    nV = np.sqrt((V * V).sum(0))
    out.update(kstar=ks, mean=ks @ alpha, var=c_ + noise_ - (V * V).sum(0))
    out.update(scale_mean=(amp * np.abs(ks)) @ A, under_mean=TINY * (1 + pre_k @ (A + 1)))
    out.update(scale_var=np.full(M, c_ + noise_), under_var=np.zeros(M, dtype=LD))
    if derivatives and kind != "matern12":
        J, sJ, uJ = (np.zeros((M, O, D), dtype=LD) for _ in range(3))
        Jvar, dvar, sdv = np.zeros((M, D), dtype=LD), np.zeros((D, M), dtype=LD), np.zeros((D, M), dtype=LD)
        for d in range(D):
            u = (Xl[:, d][None, :] - Ql[:, d][:, None]) / (lsv[d] * lsv[d])          # (M, N)
            dk = c_ * gq * u
            Vd = forward_substitution(L, np.ascontiguousarray(dk.T))
            J[:, :, d] = dk @ alpha
            sJ[:, :, d] = (amp * np.abs(dk)) @ A
            uJ[:, :, d] = TINY * (1 + (pre_g * np.abs(u)) @ (A + 1))
            Jvar[:, d] = c_ * LD(G0[kind]) / (lsv[d] * lsv[d]) - (Vd * Vd).sum(0)
            dvar[d] = LD(-2) * (Vd * V).sum(0)
            sdv[d] = LD(2) * nV * np.sqrt((Vd * Vd).sum(0))
        prior = np.broadcast_to(c_ * LD(G0[kind]) / (lsv * lsv), (M, D))
        out.update(J=J, Jvar=Jvar, dvar=dvar, scale_J=sJ, under_J=uJ, scale_Jvar=prior, scale_dvar=sdv)
        out.update(under_Jvar=np.zeros((M, D), dtype=LD), under_dvar=np.full((D, M), (2 * N + 2) * TINY, dtype=LD))
    return out


# --------------------------------------------------------------------------- the library's algebra in fp64
def posterior_float64(X, Y, c, ls, noise, jitter, kind, Xq=None, derivatives=True, gradient=True):
    """mean, var, J, Jvar, dvar, lml, grad_ard, grad_iso as the library forms them, in fp64 numpy (LAPACK Cholesky)."""
    f8 = np.float64
    N, D = X.shape
    O = Y.shape[1]
    inv = 1.0 / _full_ls(ls, D)
    Xs = X * inv
    a2, diffs = _sq(Xs, Xs)
    k, g, _, _, _ = shapes(a2, kind, f8)
    K = c * k
    K[np.diag_indices_from(K)] += noise + jitter
    L = np.linalg.cholesky(K)
    W = np.linalg.inv(L)
    alpha = W.T @ (W @ Y)
    out = {"L": L, "alpha": alpha,
           "lml": float((-0.5 * np.einsum("no,no->o", Y, alpha)).sum() - O * np.log(np.diag(L)).sum() - O * N / 2 * np.log(2 * np.pi))}
    if gradient:
        inner = alpha @ alpha.T - O * (W.T @ W)
        Gc = c * lml_shape(a2, k, g, kind)
        sums = np.array([np.sum(inner * (c * k))] + [np.sum(inner * Gc * (df * df)) for df in diffs] + [noise * np.trace(inner)]) / 2
        out["grad_ard"] = sums
        out["grad_iso"] = np.array([sums[0], sums[1:1 + D].sum(), sums[-1]])
    if Xq is None:
        return out
    # prediction kernels: coordinates carry 1 / sqrt2, so that the squared distance is h itself.  The stored sources (X (1 / l))
    # take the factor in a second multiplication, a query takes the rounded product (1 / l)(1 / sqrt2) in one: two roundings
    # of the same number, so that a query bitwise on a source is |x / l| ulps beside it, not at r = 0
    hq, dq = _sq(Xq * (inv * RS2), Xs * RS2)
    ks, cg, _, _, _ = shapes(hq + hq, kind, f8, lnc=np.log(c))
    V = W @ ks.T
    out.update(mean=ks @ alpha, var=(c + noise) - (V * V).sum(0))
    if derivatives and kind != "matern12":
        M = Xq.shape[0]
        J, Jvar, dvar = np.zeros((M, O, D)), np.zeros((M, D)), np.zeros((D, M))
        for d in range(D):
            dk = cg * dq[d] * (inv[d] * S2)
            Vd = W @ dk.T
            J[:, :, d] = dk @ alpha
            Jvar[:, d] = c * (G0[kind] * inv[d] * inv[d]) - (Vd * Vd).sum(0)
            dvar[d] = -2.0 * (Vd * V).sum(0)
        out.update(J=J, Jvar=Jvar, dvar=dvar)
    return out


# --------------------------------------------------------------------------- both, and the tolerance of every element
def _relative(err, scale):
    """Largest err / scale over the elements whose scale is a normal number (0 if there are none)."""
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    ok = scale > 2.0 ** -1000
    return float(np.max(err[ok] / scale[ok])) if np.any(ok) else 0.0


def reference(X, Y, c, ls, noise, jitter, kind, Xq=None, derivatives=True, gradient=True):
    """The longdouble results (key: float64 copy, key + "_ld": as computed) with, per output, e_rel (the fp64 restatement's
    largest deviation in units of the scale), unit = max(e_ref, floor) and tol = 16 unit, elementwise."""
    ld = posterior_longdouble(X, Y, c, ls, noise, jitter, kind, Xq, derivatives, gradient)
    f8 = posterior_float64(X, Y, c, ls, noise, jitter, kind, Xq, derivatives, gradient)
    ref = {"e_rel": {}, "unit": {}, "tol": {}, "f64": f8, "K": ld["K"].astype(np.float64)}

    def add(key, scale, under):
        ref[key + "_ld"] = ld[key]
        ref[key] = np.asarray(ld[key], dtype=np.float64)
        err = np.abs(np.asarray(f8[key], dtype=LD) - ld[key])
        scale = np.asarray(scale, dtype=np.float64)
        e_rel = _relative(err, scale)
        unit = np.maximum(e_rel, FLOOR_ULPS * EPS) * scale + np.asarray(under, dtype=np.float64)
        ref["scale_" + key], ref["e_rel"][key], ref["unit"][key], ref["tol"][key] = scale, e_rel, unit, MARGIN * unit

    ref["L"], ref["alpha"] = ld["L"].astype(np.float64), ld["alpha"].astype(np.float64)
    add("lml", ld["scale_lml"], 0.0)
    if gradient:
        add("grad_ard", ld["scale_grad_ard"], 0.0)
        add("grad_iso", ld["scale_grad_iso"], 0.0)
    if Xq is not None:
        ref["arg_min"] = ld["arg_min"]
        with np.errstate(under="ignore"):
            ref["kstar"] = ld["kstar"].astype(np.float64)   # rounded to double: exact zeros and subnormals as a double sees them
        for key in OUTPUTS:
            if key in ld:
                add(key, ld["scale_" + key], ld["under_" + key])
    for v in list(ref.values()) + list(ref["unit"].values()) + list(ref["tol"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def ratio(got, ref, key):
    """Largest |got - longdouble| / max(e_ref, floor) of the output (bound: MARGIN); 0 where both the error and the unit are 0."""
    err = np.abs(np.asarray(got, dtype=LD) - ref[key + "_ld"]).astype(np.float64)
    unit = np.broadcast_to(ref["unit"][key], err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / unit)
    return float(np.max(q)) if q.size else 0.0


def assert_within(got, ref, key, what):
    """Elementwise |got - longdouble| <= 16 max(e_ref, floor); prints and returns the largest ratio."""
    got = np.asarray(got)
    want = ref[key + "_ld"]
    assert got.shape == np.shape(want), f"{what} {key}: shape {got.shape} vs {np.shape(want)}"
    assert np.all(np.isfinite(got)), f"{what} {key}: non-finite values"
    q = ratio(got, ref, key)
    print(f"{what} {key}: err / max(e_ref, floor) = {q:.3f} (bound {MARGIN:g}; e_ref {ref['e_rel'][key]:.2e} of the scale)")
    err = np.abs(np.asarray(got, dtype=LD) - want).astype(np.float64)
    bad = np.argwhere(np.atleast_1d(err > ref["tol"][key]))
    assert bad.size == 0, (f"{what} {key}: {len(bad)} of {err.size} elements beyond 16 max(e_ref, floor), ratio {q:.3g}; "
                           f"first {bad[:5].tolist()}")
    return q


LML_CHECK_MAX_N = 400      # 80-bit numpy has no BLAS: K^-1 of 1024 points takes half a minute, of 400 about a second


def assert_lml_gradient(X, Y, c, ls, noise, jitter, kind, lml, grad, what):
    """The LML and every component of its gradient, as a fitted handle returned them, against the longdouble restatement by the
    rule above (components differ by orders of magnitude; a bound on the largest one says little about the smallest).
    Returns the largest ratio.  Where the restatement cannot be run in a test's time (more than LML_CHECK_MAX_N points) or has
    nothing to add (no extended type) it says so on the test's output and returns None: the caller's own assertions stand alone."""
    ls = np.atleast_1d(np.asarray(ls, dtype=np.float64))
    if not longdouble_is_extended():
        print(f"{what}: NOT CHECKED component by component (numpy.longdouble has eps {np.finfo(LD).eps:.1e} here)")
        return None
    if X.shape[0] > LML_CHECK_MAX_N:
        print(f"{what}: NOT CHECKED component by component ({X.shape[0]} points; the 80-bit restatement stops at {LML_CHECK_MAX_N})")
        return None
    ref = reference(X, Y, float(c), ls, float(noise), float(jitter), kind)
    key = "grad_iso" if ls.size == 1 else "grad_ard"
    return max(assert_within(np.float64(lml), ref, "lml", what), assert_within(grad, ref, key, what))
