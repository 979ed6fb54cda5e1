"""The reference's `SVGP` model (policy_transportation/models/torch/stocastic_variational_gaussian_process_derivatives.py)
on the GPU: the exact-GP prediction on pseudo-points — `convert_to_exact_gp` (:72-78), `posterior_f` (:113-129) and
`posterior_f_prime` (:132-153) — and, opt-in, the variational training of the wrapper class
`StocasticVariationalGaussianProcess` (:155-200) that the SVGP transport calls.

Prediction takes what training leaves behind — inducing points Z (Z,D), pseudo-point covariances Sigma (T,Z,Z),
pseudo-targets y (T,Z) or (T,Z,1), per-task outputscale (T,) and the ARD length-scale (D,) — and runs the prediction
algebra on the GPU: ONE handle holds all T tasks (`gpt_fit_svgp`: the tasks' inverse factors are stacked into one A
operand and share one generated kernel-column operand), factorised in fp64, predicted in fp32 (the reference's
arithmetic: it casts everything with `.float()`) or fp64.  The reference materialises M x M matrices (:120-123,
:142-144) and cannot reach M = 1e6; this path never does.

Training (`variational_training=True`; the reference's :168-187 runs it in gpytorch, which is not a dependency here):
Adam on the whitened variational ELBO, every optimiser step fused into one HIP launch pair (`gpt_svgp_train`, fp64),
then the trained q(u) is converted to pseudo-points on the host (`variational_to_pseudo_points`).  The model is a
restatement of gpytorch's defaults as read (DESIGN "SVGP training").  Its m / C structure is pinned: at the closed-form
(Titsias) optimum of q(u) the gradients vanish and the loss is the collapsed bound (tests/test_svgp_anchors.py).  Its
gpytorch constants (the 1e-4 jitter, the 1e-4 noise floor) and gpytorch's float32 numbers stay unpinned.

Parity: the prediction and the pseudo-point conversion are pinned to the reference's fixtures in the homoscedastic case
(Z = X, Sigma_t = (noise + alpha) I is the sklearn GP of tests/golden/*.npz; tests/test_svgp_anchors.py).  A general
Sigma_t and gpytorch's float32 numbers stay unpinned; there the yardstick is oracle/gp_oracle.py:svgp_exact_oracle.
Where the reference's :142 broadcasts K_inv over the input-dimension axis (it only type-checks for T == D), the intended
per-task K_inv[t] is used."""
from __future__ import annotations

import numpy as np

from . import _lib

_DTYPES = {"float32": _lib.GPT_F32, "float64": _lib.GPT_F64, np.float32: _lib.GPT_F32, np.float64: _lib.GPT_F64,
           _lib.GPT_F32: _lib.GPT_F32, _lib.GPT_F64: _lib.GPT_F64}


def _dtype_code(dtype):
    try:
        key = dtype if dtype in _DTYPES else np.dtype(dtype).name
        return _DTYPES[key]
    except (KeyError, TypeError):
        raise ValueError(f"dtype must be float32 or float64, got {dtype!r}") from None


class SVGPExactPredictor:
    def __init__(self, x_inducing, var_inducing, y_inducing, outputscale, lengthscale, device=0, dtype="float32",
                 jitter=0.0):
        Z = np.asarray(x_inducing, dtype=np.float64)
        S = np.asarray(var_inducing, dtype=np.float64)
        y = np.asarray(y_inducing, dtype=np.float64)
        if y.ndim == 3:
            y = y[:, :, 0]
        os_ = np.atleast_1d(np.asarray(outputscale, dtype=np.float64))
        T = S.shape[0]
        if Z.ndim != 2 or S.shape != (T, len(Z), len(Z)) or y.shape != (T, len(Z)) or os_.shape != (T,):
            raise ValueError("expected x_inducing (Z,D), var_inducing (T,Z,Z), y_inducing (T,Z[,1]), outputscale (T,)")
        self.num_tasks, self.n_features = T, Z.shape[1]
        self.lengthscale = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64)).reshape(-1)
        self.dtype = _dtype_code(dtype)
        self._handle = _lib.Handle(device)
        self._handle.fit_svgp(Z, y, S, self.lengthscale, os_, jitter=jitter, dtype=self.dtype)   # convert_to_exact_gp (:72-78)

    def posterior(self, x, return_std=True):
        """mean (M,T), std (M,T), Jacobian (M,T,D), Jacobian std (M,T,D) in ONE pass over the stacked factors
        (what test/svgp_derivatives_mimo.py:73-78 asks for in two calls)."""
        out = self._handle.predict_all(x, mean=True, var=bool(return_std), J=True, Jvar=bool(return_std))
        if not return_std:
            return out["mean"], out["J"]
        return out["mean"], np.sqrt(out["var"]), out["J"], np.sqrt(np.maximum(out["Jvar"], 0))

    def posterior_f(self, x, return_std=False):
        """mean (M,T) [, std (M,T)]  (:113-129).  (The reference's mean-only branch returns (T,M): it skips the permute
        of :125; here both branches use the (M,T) layout its callers rely on.)"""
        out = self._handle.predict_all(x, mean=True, var=bool(return_std))
        if not return_std:
            return out["mean"]
        return out["mean"], np.sqrt(out["var"])

    def posterior_f_prime(self, x, return_std=False):
        """Jacobian mean (M,T,D) [, its std (M,T,D)]  (:132-153)."""
        out = self._handle.predict_all(x, J=True, Jvar=bool(return_std))
        if not return_std:
            return out["J"]
        return out["J"], np.sqrt(np.maximum(out["Jvar"], 0))

    # the reference wrapper's names (StocasticVariationalGaussianProcess.predict / derivative, :189-200)
    def predict(self, x, return_std=False):
        return self.posterior_f(x, return_std=return_std)

    def derivative(self, x):
        return self.posterior_f_prime(x, return_std=True)

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None


SVGP_JITTER = 1e-4              # gpytorch's float32 Cholesky jitter (as read; unpinned)
PSEUDO_POINT_FLOOR = 1e-2       # smallest eigenvalue of I - S kept by the pseudo-point conversion (DESIGN "SVGP training")


def _softplus(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


def _rbf(a, b, ls):
    d = (a[:, None, :] - b[None, :, :]) / ls
    return np.exp(-0.5 * (d * d).sum(-1))


def svgp_schedule(n, num_epochs, batch_size=10):
    """The reference's DataLoader(batch_size, shuffle=True) (:159-160) on numpy's global RNG: a fresh permutation per
    epoch, a short last batch.  Returns (idx (num_epochs * n,), batch_begin (steps + 1,)) for gpt_svgp_train."""
    idx = np.concatenate([np.random.permutation(n) for _ in range(num_epochs)]).astype(np.int64)
    starts = np.arange(0, n, batch_size)
    bb = np.concatenate([e * n + starts for e in range(num_epochs)] + [[num_epochs * n]]).astype(np.int64)
    return idx, bb


def variational_to_pseudo_points(Z, m, C, raw_lengthscale, raw_outputscale, floor=PSEUDO_POINT_FLOOR):
    """The exact-GP form of a trained whitened q(u) (`convert_to_exact_gp`, :72-78, via gpytorch's `pseudo_points`),
    host fp64, per task t with L_t = chol(c_t k(Z,Z) + eps I) (the factor training whitens with) and S_t = C_t C_t^T:
    I - S_t = V diag(r) V^T, r+ = max(r, floor), Sigma_w = V diag(1/r+ - 1) V^T, y_w = V diag(1/r+) V^T m_t, then
    Sigma_t = L_t Sigma_w L_t^T + eps I and y_t = L_t y_w.  The exact GP on (Z, Sigma_t, y_t) has the SVGP's mean
    exactly and its variance (minus eps) wherever r >= floor; with floor = 0 and S_t < I it is gpytorch's formula with an
    exact inner solve.  The floor keeps c_t k(Z,Z) + Sigma_t positive definite when S_t has eigenvalues >= 1, which
    trained models do.  Returns the keyword arguments of set_pseudo_points."""
    Z = np.asarray(Z, np.float64)
    m = np.asarray(m, np.float64)
    C = np.asarray(C, np.float64)
    ls, c = _softplus(raw_lengthscale), _softplus(raw_outputscale)
    T, Zn = m.shape
    R = _rbf(Z, Z, ls)
    eye = np.eye(Zn)
    Sig = np.empty((T, Zn, Zn))
    y = np.empty((T, Zn))
    for t in range(T):
        L = np.linalg.cholesky(c[t] * R + SVGP_JITTER * eye)
        Ct = np.tril(C[t])
        r, V = np.linalg.eigh(eye - Ct @ Ct.T)
        rp = np.maximum(r, floor) if floor > 0 else r
        Sw = (V * (1.0 / rp - 1.0)) @ V.T
        yw = V @ ((V.T @ m[t]) / rp)
        Sig[t] = L @ Sw @ L.T + SVGP_JITTER * eye
        Sig[t] = 0.5 * (Sig[t] + Sig[t].T)
        y[t] = L @ yw
    return dict(x_inducing=Z.copy(), var_inducing=Sig, y_inducing=y, outputscale=c, lengthscale=ls)


class StocasticVariationalGaussianProcess:
    """Mirror of the reference wrapper (:155-200): `fit(num_epochs)`, `predict(x, return_std)` and `derivative(x)` over
    the exact-GP conversion of an SVGP.

    With `variational_training=True`, `fit` trains the model as the reference does (:168-187; model :15-63):
    Z = X[idx] with idx = np.random.choice(N, num_inducing) (with replacement), m_t = Y[idx, t], C_t = I, every raw
    hyper-parameter 0; Adam (lr 0.01) on the negative variational ELBO over minibatches of 10 in a fresh numpy
    permutation per epoch — every step on the GPU in fp64 (`gpt_svgp_train`), numpy's global RNG for all draws
    (`np.random.seed` makes a fit repeatable).  It keeps `loss_history_` (per step) and the trained `variational_params_`,
    converts them with `variational_to_pseudo_points` and predicts through `set_pseudo_points`.

    Without it (the default), `fit` refuses: hand trained quantities to `set_pseudo_points` instead (what
    `convert_to_exact_gp`, :72-78, reads from gpytorch: inducing points, pseudo-point covariances and targets,
    outputscales, length-scale)."""

    def __init__(self, X, Y, num_inducing=100, device=0, dtype="float32", variational_training=False):
        self.X = np.asarray(X, dtype=np.float64)
        self.Y = np.asarray(Y, dtype=np.float64)
        self.num_inducing = num_inducing
        self.device, self.dtype = device, dtype
        self.variational_training = bool(variational_training)
        self.gp = None

    def fit(self, num_epochs=10, lr=0.01, batch_size=10):
        if not self.variational_training:
            raise NotImplementedError(
                "variational training of the SVGP is off: construct with variational_training=True to train it on the "
                "GPU (reference :168-187), or pass inducing points / pseudo-point covariances / pseudo-targets / "
                "outputscales / length-scale of a model trained elsewhere to set_pseudo_points()")
        N = len(self.X)
        idx0 = np.random.choice(N, self.num_inducing)                  # :21 (with replacement)
        order, bb = svgp_schedule(N, num_epochs, batch_size)
        T, D, Zn = self.Y.shape[1], self.X.shape[1], self.num_inducing
        params = {"Z": self.X[idx0].copy(), "m": self.Y[idx0].T.copy(), "C": np.tile(np.eye(Zn), (T, 1, 1)),
                  "raw_ls": np.zeros(D), "raw_os": np.zeros(T), "raw_noise": np.zeros(T + 1)}
        self.loss_history_ = _lib.svgp_train(self.X, self.Y, params, order, bb, lr=lr, device=self.device)
        self.variational_params_ = params
        pp = variational_to_pseudo_points(params["Z"], params["m"], params["C"], params["raw_ls"], params["raw_os"])
        return self.set_pseudo_points(**pp)

    def set_pseudo_points(self, x_inducing, var_inducing, y_inducing, outputscale, lengthscale, jitter=0.0):
        if self.gp is not None:
            self.gp.close()
        self.gp = SVGPExactPredictor(x_inducing, var_inducing, y_inducing, outputscale, lengthscale, device=self.device,
                                     dtype=self.dtype, jitter=jitter)
        return self

    def _require(self):
        if self.gp is None:
            raise RuntimeError("StocasticVariationalGaussianProcess has no model: call set_pseudo_points() first")
        return self.gp

    def predict(self, x, return_std=False):
        return self._require().posterior_f(x, return_std=return_std)

    def derivative(self, x):
        return self._require().posterior_f_prime(x, return_std=True)
