"""GaussianProcessBatch — many small independent GaussianProcess models (n <= 128 points each) fitted, optimised and
evaluated together: one workgroup per model, one launch per operation (gpt_batch_* of include/gpt_hip.h).

The reference fits one transport per frame pair on about ten source points, hundreds of times in a loop
(example/comparisons/multi_reference_frames/models/model_gpt.py:74-83).  Every member of the batch gets the numbers,
shapes and quirks GaussianProcess gives one model (policy_transportation/models/gaussian_process.py:16-126); the methods
take and return one entry per model."""
from __future__ import annotations

import copy

import numpy as np

from . import _lib
from .gaussian_process import _PARAM_C, _PARAM_LS, _PARAM_NOISE, kernel_hyperparameters, kernel_type


class GaussianProcessBatch:
    def __init__(self, kernel, alpha=1e-10, optimizer="fmin_l_bfgs_b", n_restarts_optimizer=5, device=0, verbose=False):
        """Arguments as GaussianProcess's; `kernel` (ConstantKernel * RBF or Matern + WhiteKernel) is every model's starting
        point.  A callable optimizer is refused (batch_hyperopt.py).  optimizer="device_bfgs" (opt-in) runs the search itself
        on the device, one workgroup per (model, start point): same start points and restarts, a projected BFGS iteration in
        place of scipy's L-BFGS-B; optimizer_stats_ then holds runs, launches and evaluations."""
        from .batch_hyperopt import check_optimizer
        check_optimizer(optimizer)
        self._kernel_in = kernel
        self.kernel = kernel
        self.alpha = alpha
        self.optimizer = optimizer
        self.n_restarts_optimizer = n_restarts_optimizer if optimizer is not None else 0
        self.device = device
        self.verbose = verbose
        self._fitted = False

    # ------------------------------------------------------------------ fit
    def fit(self, Xs, Ys):
        """Xs, Ys: sequences of (n_b, D) / (n_b, O) arrays (a 1-D y is one output).  Rows whose target holds NaN are dropped
        per model, as GaussianProcess.fit does (gaussian_process.py:33-35)."""
        Xs, Ys = list(Xs), list(Ys)
        if len(Xs) != len(Ys):
            raise ValueError(f"GaussianProcessBatch.fit: {len(Xs)} inputs but {len(Ys)} targets")
        X_f, Y_f = [], []
        for b, (X, Y) in enumerate(zip(Xs, Ys)):
            X = np.asarray(X, dtype=np.float64)
            Y = np.asarray(Y, dtype=np.float64)
            if Y.ndim == 1:
                Y = Y[:, None]
            if X.ndim != 2 or Y.ndim != 2:
                raise ValueError(f"GaussianProcessBatch.fit: model {b}: expected 2-D arrays, got shapes {X.shape} and {Y.shape}")
            if X.shape[0] != Y.shape[0]:
                raise ValueError(f"GaussianProcessBatch.fit: model {b}: X and Y have different numbers of rows")
            mask = np.isnan(Y).any(axis=1)
            X, Y = X[~mask], Y[~mask]
            if X.shape[0] > _lib.BATCH_MAX_N:
                raise ValueError(f"GaussianProcessBatch.fit: model {b} has {X.shape[0]} rows after the NaN filter; a batch member "
                                 f"holds at most {_lib.BATCH_MAX_N} points.  Fit larger models with GaussianProcess")
            X_f.append(X)
            Y_f.append(Y)
        _lib.batch_pack(X_f, Y_f, "GaussianProcessBatch.fit")      # every refusal that needs no device
        self.Xs, self.Ys = X_f, Y_f
        B = len(X_f)
        self.n_models = B
        self.n_features = X_f[0].shape[1]
        self.n_outputs = Y_f[0].shape[1]
        c0, ls0, noise0 = kernel_hyperparameters(self._kernel_in)
        self._ktype = kernel_type(self._kernel_in)
        if ls0.size not in (1, self.n_features):                  # before the search, as the single-model class fails before any device work
            raise ValueError(f"GaussianProcessBatch.fit: the kernel's length_scale has {ls0.size} entries, the models have "
                             f"{self.n_features} features (1 or D entries are accepted)")
        hyper = [(c0, ls0, noise0, None)] * B
        if self.optimizer is not None:
            from .batch_hyperopt import optimize_hyperparameters_batch
            self.optimizer_stats_ = {}
            hyper = optimize_hyperparameters_batch(self._kernel_in, X_f, Y_f, self.alpha, self.optimizer, self.n_restarts_optimizer,
                                                   self._ktype, self.device, self.optimizer_stats_)
        self._c = np.array([h[0] for h in hyper])
        self._ls = np.array([h[1] for h in hyper])
        self._noise = np.array([h[2] for h in hyper])
        L, a, lml, status = _lib.batch_fit(X_f, Y_f, self._ls, self._c, self._noise, self.alpha, self._ktype, self.device)
        bad = [int(b) for b in np.flatnonzero(status != _lib.GPT_OK)]
        if bad:
            raise np.linalg.LinAlgError(f"GaussianProcessBatch.fit: the kernel matrix of model(s) {bad} is not positive definite at the "
                                        "fitted hyper-parameters (non-positive pivot); increase alpha or the noise level")
        self.L_, self.alpha_ = L, a
        self.log_marginal_likelihood_values_ = lml
        keep_array = np.iterable(self._kernel_in.get_params()[_PARAM_LS])
        self.kernels_ = []
        for b in range(B):
            k = copy.deepcopy(self._kernel_in)
            k.set_params(**{_PARAM_C: float(self._c[b]), _PARAM_LS: (self._ls[b].copy() if keep_array else float(self._ls[b][0])),
                            _PARAM_NOISE: float(self._noise[b])})
            self.kernels_.append(k)
        self._fitted = True
        if self.verbose:
            for b, k in enumerate(self.kernels_):
                print("model", b, "lenghtscales", k.get_params()[_PARAM_LS])
        return self

    def _posterior(self, xs, what, **want):
        if not self._fitted:
            raise RuntimeError("GaussianProcessBatch is not fitted")
        xs = list(xs)
        if len(xs) != self.n_models:
            raise ValueError(f"GaussianProcessBatch.{what}: {len(xs)} query arrays for {self.n_models} models")
        if self._ktype != 0 and (want.get("J") or want.get("Jvar") or want.get("dvar")):
            raise NotImplementedError(f"GaussianProcessBatch.{what}: derivatives of a batch are RBF only; "
                                      "GaussianProcess(..., matern_derivatives=True) has the analytic Matern derivatives")
        out, status = _lib.batch_predict(self.Xs, self.Ys, self._ls, self._c, self._noise, self.alpha, xs, self._ktype, self.device,
                                         **want)
        return out

    # ------------------------------------------------------------------ one member's results in GaussianProcess's shapes
    def _member_predict(self, b, mean, var=None):
        if self.n_outputs == 1:
            mean = mean[:, 0]                       # sklearn squeezes single-target output (_gpr.py:449-451)
        if var is None:
            return mean
        std = np.sqrt(var)
        if self.n_outputs > 1:
            std = np.repeat(std[:, None], self.n_outputs, axis=1)   # _gpr.py:488
        return mean, std - np.sqrt(self._noise[b])  # reference quirk (gaussian_process.py:49)

    def _member_derivative(self, b, J, Jvar=None):
        if Jvar is None:
            return J
        return J, np.repeat(Jvar[:, None, :], self.n_outputs, axis=1)

    # ------------------------------------------------------------------ predict
    def predict(self, xs, return_std=False):
        """Per model what GaussianProcess.predict returns (:46-55): mean (M_b, O), squeezed for a single output; with
        return_std also `std - sqrt(noise_level)` tiled over the outputs."""
        out = self._posterior(xs, "predict", mean=True, var=bool(return_std))
        return [self._member_predict(b, out["mean"][b], out["var"][b] if return_std else None) for b in range(self.n_models)]

    def derivative(self, xs, return_var=False):
        """Per model J (M_b, O, D); with return_var also its variance tiled over the outputs (M_b, O, D) (:63-102)."""
        out = self._posterior(xs, "derivative", J=True, Jvar=bool(return_var))
        return [self._member_derivative(b, out["J"][b], out["Jvar"][b] if return_var else None) for b in range(self.n_models)]

    def derivative_of_variance(self, xs):
        """Per model the (D, M_b) array of d var / d x_d (:104-126)."""
        out = self._posterior(xs, "derivative_of_variance", dvar=True)
        return [np.ascontiguousarray(g.T) for g in out["dvar"]]

    def posterior(self, xs, jacobian_variance=False):
        """Per model a dict with mean (M_b, O), raw variance (M_b,), Jacobian (M_b, O, D) [and its variance (M_b, D)], from
        one call — GaussianProcess.posterior."""
        out = self._posterior(xs, "posterior", mean=True, var=True, J=True, Jvar=bool(jacobian_variance))
        return [{k: v[b] for k, v in out.items()} for b in range(self.n_models)]
