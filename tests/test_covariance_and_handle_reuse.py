"""Two parts of the exact-GP library that sit on the fit-side state of a handle.

A. gpt_predict_cov past one query tile, against an extended-precision restatement (numpy.longdouble: kernel matrix, column-loop
   Cholesky, forward substitution, cov = k(Xq,Xq) + noise I - V^T V), elementwise over the whole M x M matrix.  The tolerance is
   16 x max(e_ref, 64 x 2^-52 x (c + noise)), where e_ref is the deviation of an fp64 numpy restatement of the library's own
   algebra (explicit W = L^-1, V = W K*) from the longdouble result: the rounding floor of the operation itself, measured in the
   test and never taken from the library.  16 is the margin for the other summation order (MFMA blocks of 4, a blocked inverse):
   constants, not orders of magnitude, while an indexing or stride fault moves entries by 1e-3 .. 1.

B. One handle through a sequence of models (smaller, same padded size, other D / O / kernel / dtype / model kind, failed fits)
   must give, after every fit, bitwise what a handle created for that fit alone gives.

The restatement tests run anywhere; the tests that run the library need an MI355X."""
import functools

import numpy as np
import pytest

LD = np.longdouble
EPS = 2.0 ** -52
C0 = 1.3                                   # constant_value of every covariance case
JITTER = 1e-10
KINDS = ("rbf", "matern12", "matern32", "matern52")        # index = kernel_type of the C ABI

# (N, M, D, kernel_type, O, isotropic, noise): the smallest shapes that cross each boundary of the covariance path
#   Mp = ceil(M / 128) * 128 is the padded query count; k_cross_t runs Mp / 64 x NP / 64 workgroups
COV_CASES = [
    (1, 1, 1, 0, 1, False, 1e-2),          # degenerate sizes
    (63, 63, 3, 0, 2, False, 1e-2),        # inside one tile
    (63, 64, 2, 2, 2, False, 1e-2),        # tile exactly full
    (300, 65, 3, 0, 2, True, 1e-2),        # first query in tile 1
    (300, 128, 3, 3, 2, False, 1e-2),      # Mp == M
    (300, 129, 1, 1, 2, False, 1e-3),      # Mp 128 -> 256
    (600, 200, 3, 0, 5, False, 1e-2),      # NP past 512, two output passes
    (300, 385, 5, 3, 2, False, 1e-2),      # Mp = 512, row-of-8 layout
    (600, 129, 12, 2, 2, False, 1e-2),     # row-of-16 layout
    (600, 257, 15, 0, 2, False, 1e-2),     # Mp = 384, D at its limit
]
COV_IDS = [f"N{c[0]}-M{c[1]}-D{c[2]}-{KINDS[c[3]]}" for c in COV_CASES]


# --------------------------------------------------------------------------- the restatements
def kernel_matrix(A, B, ls, c, kind, dtype):
    """c k(|(a - b) / ls|) with sklearn's formulas (kernels.py: RBF 1553-1565, Matern 1717-1745), in `dtype`."""
    A = np.asarray(A, dtype=dtype) / np.asarray(ls, dtype=dtype)
    B = np.asarray(B, dtype=dtype) / np.asarray(ls, dtype=dtype)
    d2 = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
    for d in range(A.shape[1]):
        df = A[:, d][:, None] - B[:, d][None, :]
        d2 += df * df
    if kind == "rbf":
        k = np.exp(-d2 / dtype(2))
    else:
        r = np.sqrt(d2)
        if kind == "matern12":
            k = np.exp(-r)
        elif kind == "matern32":
            t = r * np.sqrt(dtype(3))
            k = (dtype(1) + t) * np.exp(-t)
        elif kind == "matern52":
            t = r * np.sqrt(dtype(5))
            k = (dtype(1) + t + t * t / dtype(3)) * np.exp(-t)
        else:
            raise ValueError(kind)
    return dtype(c) * k


def cholesky_columns(K):
    """Lower Cholesky factor by the column loop, in K's own precision."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        row = L[j, :j]
        L[j, j] = np.sqrt(K[j, j] - row @ row)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ row) / L[j, j]
    return L


def forward_substitution(L, B):
    """L \\ B for lower-triangular L, row by row, in L's precision."""
    V = np.zeros_like(B)
    for i in range(L.shape[0]):
        V[i] = (B[i] - L[i, :i] @ V[:i]) / L[i, i]
    return V


def posterior_longdouble(X, Y, Xq, ls, c, noise, jitter, kind):
    """(mean, cov) of the exact GP in 80-bit arithmetic; the training diagonal carries noise + jitter, the predictive one noise."""
    K = kernel_matrix(X, X, ls, c, kind, LD)
    K[np.diag_indices_from(K)] += LD(noise) + LD(jitter)
    L = cholesky_columns(K)
    Ks = kernel_matrix(X, Xq, ls, c, kind, LD)                      # (N, M)
    V = forward_substitution(L, Ks)
    cov = kernel_matrix(Xq, Xq, ls, c, kind, LD) - V.T @ V
    cov[np.diag_indices_from(cov)] += LD(noise)
    # alpha = L^-T L^-1 Y, mean = K*^T alpha
    z = forward_substitution(L, np.asarray(Y, dtype=LD))
    alpha = forward_substitution(L.T[::-1, ::-1], z[::-1])[::-1]
    return Ks.T @ alpha, cov


def posterior_float64_inverse(X, Y, Xq, ls, c, noise, jitter, kind):
    """The library's algebra in fp64 numpy: W = L^-1 formed explicitly, V = W K*, alpha = W^T (W Y)."""
    f8 = np.float64
    K = kernel_matrix(X, X, ls, c, kind, f8)
    K[np.diag_indices_from(K)] += noise + jitter
    W = np.linalg.inv(np.linalg.cholesky(K))
    Ks = kernel_matrix(X, Xq, ls, c, kind, f8)
    V = W @ Ks
    cov = kernel_matrix(Xq, Xq, ls, c, kind, f8) - V.T @ V
    cov[np.diag_indices_from(cov)] += noise
    return Ks.T @ (W.T @ (W @ Y)), cov


def smooth_targets(X, O, rng):
    """Smooth in X plus small noise, as in the golden fixtures."""
    cols = [0.05 * np.sin(4.0 * X[:, o % X.shape[1]] + o) for o in range(O)]
    return np.stack(cols, axis=1) + 0.01 * rng.standard_normal((X.shape[0], O))


def cov_queries(X, M, rng):
    """Uniform on [-0.1, 1.1]^D; the first 8 are training points (the diagonal cancels down to about the noise), query 11 is
    an exact duplicate of query 10 (its off-diagonal entry is k(0) = c without the noise term), the last one sits at +50 in
    every coordinate (its row is zero off the diagonal and c + noise on it)."""
    N, D = X.shape
    Xq = rng.uniform(-0.1, 1.1, (M, D))
    n = min(8, N, M)
    Xq[:n] = X[:n]
    if M >= 13:
        Xq[11] = Xq[10]
        Xq[M - 1] = 50.0
    return Xq


@functools.lru_cache(maxsize=None)
def cov_case(i):
    """Inputs and both restatements of case i, computed once per process and shared by every test that needs them."""
    N, M, D, ktype, O, iso, noise = COV_CASES[i]
    rng = np.random.default_rng(1000 + i)
    X = rng.uniform(0.0, 1.0, (N, D))
    Y = smooth_targets(X, O, rng)
    Xq = cov_queries(X, M, rng)
    # length-scales that keep the condition number of K near 1e4 .. 2e5: they grow with sqrt(D) as the distances do
    base = 0.3 * np.sqrt(D / 3.0) if D > 3 else 0.3
    ls = np.array([base]) if iso else base * np.linspace(0.8, 1.3, D)
    full_ls = np.full(D, ls[0]) if iso else ls
    kind = KINDS[ktype]
    mean_ld, cov_ld = posterior_longdouble(X, Y, Xq, full_ls, C0, noise, JITTER, kind)
    mean_64, cov_64 = posterior_float64_inverse(X, Y, Xq, full_ls, C0, noise, JITTER, kind)
    e_ref = float(np.max(np.abs(cov_64 - cov_ld)))
    e_mean = float(np.max(np.abs(mean_64 - mean_ld)))
    tol = 16.0 * max(e_ref, 64.0 * EPS * (C0 + noise))
    out = dict(N=N, M=M, D=D, O=O, ktype=ktype, kind=kind, noise=noise, X=X, Y=Y, Xq=Xq, ls=ls, full_ls=full_ls,
               mean_ld=mean_ld, cov_ld=cov_ld, mean_64=mean_64, cov_64=cov_64, e_ref=e_ref, e_mean=e_mean, tol=tol)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# --------------------------------------------------------------------------- A, on the CPU: the reference checks itself
@pytest.mark.parametrize("i", range(len(COV_CASES)), ids=COV_IDS)
def test_restatements_agree(i):
    """The fp64 restatement and the oracle's gpr_predict(return_cov=True) (a triangular solve) agree with the longdouble one
    at the scale of e_ref, and e_ref <= 1e-12 (c + noise): the inputs are well enough conditioned for the GPU bound to bite."""
    from oracle import gp_oracle as orc
    g = cov_case(i)
    scale = C0 + g["noise"]
    print(f"{COV_IDS[i]}: e_ref {g['e_ref']:.3e} ({g['e_ref'] / scale:.3e} of c + noise), e_mean {g['e_mean']:.3e}, tol {g['tol']:.3e}")
    assert g["e_ref"] <= 1e-12 * scale
    assert np.all(np.isfinite(g["cov_ld"].astype(np.float64)))
    L, a = orc.gpr_fit(g["X"], g["Y"], C0, g["full_ls"], g["noise"], JITTER, kind=g["kind"])
    mean_o, cov_o = orc.gpr_predict(g["Xq"], g["X"], L, a, C0, g["full_ls"], g["noise"], return_cov=True, kind=g["kind"])
    if cov_o.ndim == 3:                                    # tiled over the targets
        assert all(np.array_equal(cov_o[..., 0], cov_o[..., o]) for o in range(cov_o.shape[2]))
        cov_o = cov_o[..., 0]
    err = float(np.max(np.abs(cov_o - g["cov_ld"])))
    print(f"    oracle: cov error {err:.3e} = {err / (g['tol'] / 16.0):.2f} x max(e_ref, floor)")
    assert err <= g["tol"]
    # the mean's own floor: the fp64 restatement's deviation, or 64 ulps of the largest |K*^T| |alpha| sum behind an entry
    mag = float(np.max(np.abs(kernel_matrix(g["Xq"], g["X"], g["full_ls"], C0, g["kind"], np.float64)) @ np.abs(a)))
    tol_mean = 16.0 * max(g["e_mean"], 64.0 * EPS * mag)
    assert float(np.max(np.abs(mean_o - g["mean_ld"]))) <= tol_mean
    assert float(np.max(np.abs(g["mean_64"] - g["mean_ld"]))) <= tol_mean
    # the properties the GPU test asserts hold for the reference itself
    cov = g["cov_ld"]
    assert float(np.max(np.abs(cov - cov.T))) <= 2 * g["tol"]
    if g["M"] >= 13:
        f = g["M"] - 1
        off = np.delete(cov[f], f)
        assert float(np.max(np.abs(off))) <= g["tol"] and abs(float(cov[f, f]) - scale) <= g["tol"]
        assert abs(float(cov[10, 10] - cov[10, 11]) - g["noise"]) <= g["tol"]
        assert float(np.min(np.diag(cov)[:8])) < 3 * g["noise"]          # training points: the prior variance has cancelled


# --------------------------------------------------------------------------- A, on the GPU
def fitted_handle(g):
    from gaussian_process_transportation_amd import _lib
    h = _lib.Handle(0)
    h.fit(g["X"], g["Y"], g["ls"], C0, g["noise"], JITTER, kernel_type=g["ktype"])
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(COV_CASES)), ids=COV_IDS)
def test_covariance_against_longdouble(i):
    """Largest err / max(e_ref, floor) seen on the MI355X: DESIGN.md, testing section."""
    g = cov_case(i)
    M, noise, tol = g["M"], g["noise"], g["tol"]
    h = fitted_handle(g)
    try:
        mean, cov = h.predict_cov(g["Xq"])
        out = h.predict_all(g["Xq"], mean=True, var=True)
    finally:
        h.close()
    assert cov.shape == (M, M) and np.all(np.isfinite(cov))
    err = np.abs(cov - g["cov_ld"]).astype(np.float64)
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    print(f"{COV_IDS[i]}: cov error {err.max():.3e} at {worst}, e_ref {g['e_ref']:.3e}, "
          f"ratio err / max(e_ref, floor) = {err.max() / (tol / 16.0):.3f} (bound 16)")
    bad = np.argwhere(err > tol)
    assert bad.size == 0, f"{len(bad)} of {M * M} entries beyond {tol:.3e}; first {bad[:5].tolist()}, worst {err.max():.3e} at {worst}"
    assert float(np.max(np.abs(cov - cov.T))) <= 2 * tol
    assert float(np.max(np.abs(np.diag(cov) - out["var"]))) <= tol
    assert np.array_equal(mean, out["mean"])
    assert float(np.linalg.eigvalsh(0.5 * (cov + cov.T)).min()) >= -M * tol
    if M >= 13:
        others = np.ones(M, dtype=bool)
        others[[10, 11]] = False
        assert float(np.max(np.abs(cov[10, others] - cov[11, others]))) <= tol          # the duplicate: same row,
        assert abs(cov[10, 11] - float(g["cov_ld"][10, 11])) <= tol                       # k(0) = c off the diagonal,
        assert abs((cov[10, 10] - cov[10, 11]) - noise) <= tol and abs((cov[11, 11] - cov[11, 10]) - noise) <= tol   # no noise term there
        f = M - 1
        assert float(np.max(np.abs(np.delete(cov[f], f)))) <= tol and abs(cov[f, f] - (C0 + noise)) <= tol


@pytest.mark.gpu
def test_covariance_scratch_is_not_carried_between_calls():
    """cov_buf is grow-only and laid out per call: M = 385, then 12, then 385 on one handle."""
    g = cov_case(7)
    assert g["M"] == 385
    h = fitted_handle(g)
    fresh = fitted_handle(g)
    try:
        m1, c1 = h.predict_cov(g["Xq"])
        m2, c2 = h.predict_cov(g["Xq"][:12])
        m3, c3 = h.predict_cov(g["Xq"])
        mf, cf = fresh.predict_cov(g["Xq"][:12])
        assert np.array_equal(c1, c3) and np.array_equal(m1, m3)
        assert np.array_equal(c2, cf) and np.array_equal(m2, mf)
        assert float(np.max(np.abs(c2 - g["cov_ld"][:12, :12]))) <= g["tol"]
        m0, c0 = h.predict_cov(np.zeros((0, g["D"])))
        assert m0.shape == (0, g["O"]) and c0.shape == (0, 0)
        with pytest.raises(ValueError, match="16384"):          # GPT_E_ARG; the host arrays of the call are never touched
            h.predict_cov(np.zeros((16385, g["D"])))
        m4, c4 = h.predict_cov(g["Xq"][:12])                    # and the refusal left the handle as it was
        assert np.array_equal(c4, c2) and np.array_equal(m4, m2)
    finally:
        h.close()
        fresh.close()


# --------------------------------------------------------------------------- B: one handle, many models
LS3 = np.array([0.25, 0.32, 0.4])
NOISE = 1e-2


def reuse_data(N, D, O, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, D))
    return X, smooth_targets(X, O, rng)


def reuse_queries(M, D):
    return np.random.default_rng(7000 + 31 * M + D).uniform(-0.05, 1.05, (M, D))


def spd_noise(N, T, seed):
    """Dense SPD (T, N, N), about 1e-2 on the diagonal."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((T, N, N))
    return 1e-2 * (A @ A.transpose(0, 2, 1) / N + np.eye(N))


class Step:
    """One fit: apply(h) performs it on a handle, observe(h) collects everything that model kind offers."""

    def __init__(self, name, kind, X, Y, ls=LS3, c=C0, noise=NOISE, ktype=0, dtype=None, Sigma=None, osc=None, matern_derivatives=False,
                 sizes=(700, 70), cov_size=130):
        self.name, self.kind, self.X, self.Y, self.ls, self.c, self.noise, self.ktype = name, kind, X, Y, np.asarray(ls, dtype=float), c, noise, ktype
        self.dtype, self.Sigma, self.osc, self.matern_derivatives, self.sizes, self.cov_size = dtype, Sigma, osc, matern_derivatives, sizes, cov_size

    def apply(self, h):
        from gaussian_process_transportation_amd import _lib
        h.set_matern_derivatives(self.matern_derivatives)
        h.set_dtype(_lib.GPT_F32 if self.dtype == "f32" else _lib.GPT_F64)
        if self.kind == "fit":
            h.fit(self.X, self.Y, self.ls, self.c, self.noise, JITTER, kernel_type=self.ktype)
        elif self.kind == "noise_matrix":
            h.fit_noise_matrix(self.X, self.Y, self.ls, self.c, self.Sigma, JITTER, kernel_type=self.ktype)
        elif self.kind == "svgp":
            h.fit_svgp(self.X, self.Y, self.Sigma, self.ls, self.osc, jitter=JITTER)
        elif self.kind == "objective":
            return h.lml_objective(self.X, self.Y, self.ls, self.c, self.noise, JITTER, kernel_type=self.ktype)
        else:
            raise ValueError(self.kind)
        return None

    def observe(self, h):
        from gaussian_process_transportation_amd import _lib
        D = self.X.shape[1]
        exact = self.kind in ("fit", "noise_matrix")
        got = {}
        if exact:
            got["L"], got["alpha"] = h.export()
            got["W"] = h.export_inverse_factor()
            got["lml"] = np.array(h.lml())
        else:
            got["alpha"] = h.export(want_L=False)[1]
        # derivatives: RBF always; Matern 3/2 and 5/2 once enabled; never Matern 1/2.  dvar: the single-task model only.
        deriv = self.ktype == 0 or (self.ktype in (2, 3) and self.matern_derivatives)
        for M in self.sizes:          # 70 queries take the small-batch plan of the variance kernel, 700 the general one
            out = h.predict_all(reuse_queries(M, D), mean=True, var=True, J=deriv, Jvar=deriv, dvar=deriv and exact)
            got.update({f"{k}@{M}": v for k, v in out.items() if v is not None})
        if exact and self.dtype != "f32":
            got["cov_mean"], got["cov"] = h.predict_cov(reuse_queries(self.cov_size, D))
        if exact:
            v, grad = h.lml_gradient(self.ls.size)               # last: K^-1 overwrites L
            got["lml_of_gradient"], got["gradient"] = np.array(v), grad
            with pytest.raises(_lib.GptError):
                h.export(want_L=True, want_alpha=False)
            if "cov" in got:                                     # W is still valid
                again = h.predict_cov(reuse_queries(self.cov_size, D))[1]
                assert np.array_equal(again, got["cov"]), f"{self.name}: predict_cov changed after lml_gradient"
        return got


def run_step(h, step, failures):
    """The fit on the long-lived handle and on a handle of its own; every output must agree to the bit."""
    from gaussian_process_transportation_amd import _lib
    fresh = _lib.Handle(0)
    try:
        r_h, r_f = step.apply(h), step.apply(fresh)
        if step.kind == "objective":
            got, ref = {"lml": np.array(r_h[0]), "gradient": r_h[1]}, {"lml": np.array(r_f[0]), "gradient": r_f[1]}
        else:
            got, ref = step.observe(h), step.observe(fresh)
    finally:
        fresh.close()
    assert got.keys() == ref.keys()
    for k in ref:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (step.name, k)
        assert np.all(np.isfinite(b)), (step.name, k)
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            failures.append(f"{step.name}: {k} differs from a fresh handle's in {int((a != b).sum())} of {a.size} entries (max {d.max():.3e})")
    print(f"{step.name}: {len(ref)} outputs compared" + ("" if not failures else f" ({len(failures)} mismatches so far)"))


@pytest.mark.gpu
def test_one_handle_through_many_models_equals_a_fresh_handle_each_time():
    """Every mismatch of the whole sequence is reported, not the first one only: a stale buffer tends to show in several places."""
    from gaussian_process_transportation_amd import _lib
    X1, Y1 = reuse_data(600, 3, 5, 11)
    X2, Y2 = reuse_data(300, 3, 5, 12)
    X3, Y3 = reuse_data(280, 3, 2, 13)
    Y5 = Y3.copy()
    Y5[137, 1] += 0.25
    X6 = np.ascontiguousarray(X3.reshape(420, 2))
    Y6 = smooth_targets(X6, 2, np.random.default_rng(16))
    T = 3
    y_t = np.ascontiguousarray(smooth_targets(X3, T, np.random.default_rng(21)).T)
    Sig_t = spd_noise(280, T, 22)
    Sig = spd_noise(280, 1, 23)[0]
    X13 = X3.copy()
    # identical rows, no noise, no jitter: singular.  One identical pair is not enough in floating point: its pivot is 0 in exact
    # arithmetic and comes out as +-1e-16, positive as often as not (test_not_positive_definite_in_a_late_panel); after the first
    # such pivot the column is divided by its root and a later pair's pivot is negative beyond any rounding.
    X13[200:] = X13[:80]
    X14, Y14 = reuse_data(280, 12, 2, 14)
    ls14 = np.linspace(0.6, 0.9, 12)
    X15, Y15 = reuse_data(1100, 3, 3, 15)
    X1p, Y1p = reuse_data(1, 3, 3, 17)
    base = Step("3: N 280, O 2 at the padded size of step 2 (workspace kept, npass drops)", "fit", X3, Y3)
    failures = []
    h = _lib.Handle(0)

    def must_refuse_prediction():
        with pytest.raises(_lib.GptError):
            h.predict_all(reuse_queries(5, 3), mean=True)

    try:
        run_step(h, Step("1: N 600, O 5 (padded size past 512, two output passes)", "fit", X1, Y1), failures)
        assert h.info() == (600, 3, 5, 1024)
        run_step(h, Step("2: N 300, O 5 (smaller padded size: workspace rebuilt, scratch larger than needed)", "fit", X2, Y2), failures)
        assert h.info() == (300, 3, 5, 512)
        run_step(h, base, failures)
        assert h.info() == (280, 3, 2, 512)
        run_step(h, Step("4: same X and Y, new length-scales and c (both mirrors match)", "fit", X3, Y3, ls=[0.31, 0.22, 0.45], c=0.7), failures)
        run_step(h, Step("5: same X, one element of Y changed", "fit", X3, Y5, ls=[0.31, 0.22, 0.45], c=0.7), failures)
        run_step(h, Step("6: the same doubles as (420, 2)", "fit", X6, Y6, ls=[0.3, 0.4]), failures)
        run_step(h, base, failures)
        run_step(h, Step("7a: Matern 5/2 with its derivatives", "fit", X3, Y3, ktype=3, matern_derivatives=True), failures)
        run_step(h, Step("7b: RBF again", "fit", X3, Y3, matern_derivatives=True), failures)
        run_step(h, Step("8a: lml_objective", "objective", X3, Y3), failures)
        must_refuse_prediction()                          # the objective leaves no model behind
        run_step(h, Step("8b / 9: fit after lml_objective; L is back after lml_gradient", "fit", X3, Y3), failures)
        run_step(h, Step("10a: fp32 model at the same shape", "fit", X3, Y3, dtype="f32"), failures)
        assert h.model_info() == (1, _lib.GPT_F32)
        run_step(h, Step("10b: fp64 again", "fit", X3, Y3), failures)
        run_step(h, Step("11a: fit_svgp, 3 tasks on 280 inducing points", "svgp", X3, y_t, Sigma=Sig_t, osc=np.array([1.3, 0.6, 0.9])), failures)
        assert h.model_info() == (T, _lib.GPT_F64)
        run_step(h, Step("11b: plain fit of the X and Y fitted before fit_svgp (the Y mirror must be gone)", "fit", X3, Y3), failures)
        run_step(h, Step("12a: fit_noise_matrix, dense SPD Sigma", "noise_matrix", X3, Y3, Sigma=Sig), failures)
        run_step(h, Step("12b: plain fit of the same X and Y", "fit", X3, Y3), failures)
        with pytest.raises(np.linalg.LinAlgError):       # GPT_E_NOT_PD: an error code of the factorisation, not a device fault
            h.fit(X13, Y3, LS3, C0, 0.0, 0.0)
        must_refuse_prediction()
        run_step(h, Step("13: the last good X and Y after a fit that was not positive definite", "fit", X3, Y3), failures)
        run_step(h, Step("14a: D 12 at the same padded size (source rows of 16)", "fit", X14, Y14, ls=ls14), failures)
        run_step(h, Step("14b: D 3 again (rows of 4)", "fit", X3, Y3), failures)
        run_step(h, Step("15a: N 1100 (growth after all of the above)", "fit", X15, Y15), failures)
        assert h.info() == (1100, 3, 3, 1536)
        run_step(h, Step("15b: N 1, M 5", "fit", X1p, Y1p, sizes=(5,), cov_size=5), failures)
    finally:
        h.close()
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_prediction_cache_follows_the_model():
    """The variance scratch and its cached work plan are keyed by the launch shape: reserve at N 1100, refit at N 300, and a
    replica that takes over a handle which held the larger model."""
    from gaussian_process_transportation_amd import _lib
    Xa, Ya = reuse_data(1100, 3, 3, 31)
    Xb, Yb = reuse_data(300, 3, 3, 32)
    q5000, q70 = reuse_queries(5000, 3), reuse_queries(70, 3)
    outputs = dict(mean=True, var=True, J=True, Jvar=True, dvar=True)

    def fresh(X, Y, q):
        f = _lib.Handle(0)
        try:
            f.fit(X, Y, LS3, C0, NOISE, JITTER)
            return f.predict_all(q, **outputs)
        finally:
            f.close()

    def same(got, ref, what):
        for k in ref:
            assert np.array_equal(got[k], ref[k]), f"{what}: {k} differs from a fresh handle's"

    h, h2 = _lib.Handle(0), _lib.Handle(0)
    try:
        h.fit(Xa, Ya, LS3, C0, NOISE, JITTER)
        h.reserve(5000, True)
        big = fresh(Xa, Ya, q5000)
        same(h.predict_all(q5000, **outputs), big, "N 1100 after reserve")
        h2.fit(Xa, Ya, LS3, C0, NOISE, JITTER)
        same(h2.predict_all(q5000, **outputs), big, "second handle, N 1100")
        h.fit(Xb, Yb, LS3, C0, NOISE, JITTER)
        ref5000, ref70 = fresh(Xb, Yb, q5000), fresh(Xb, Yb, q70)
        same(h.predict_all(q5000, **outputs), ref5000, "N 300 after N 1100, M 5000")
        same(h.predict_all(q70, **outputs), ref70, "N 300 after N 1100, M 70")
        h2.factor_copy_from(h)
        assert h2.info() == h.info()
        same(h2.predict_all(q5000, **outputs), ref5000, "replica over the N 1100 model, M 5000")
        same(h2.predict_all(q70, **outputs), ref70, "replica over the N 1100 model, M 70")
    finally:
        h.close()
        h2.close()
