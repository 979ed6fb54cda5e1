"""ActiveLearningGaussianProcess — the reference's large-input regressor
(policy_transportation/models/gaussian_process_al.py:15-75) on an MI355X: an exact GP that accepts more points than it
should hold and reduces them to `n_samples_max` by greedy active learning before the fit.

The reference's loop (:26-57) starts from a random 10 % of the budget and then, `n_samples_max - n_initial` times, refits
a regressor on the points chosen so far, predicts the standard deviation of every remaining pool point and moves the
largest one into the subset.  With the hyper-parameters fixed that is a pivoted Cholesky factorisation of the pool's
kernel matrix (the residual diagonal is the posterior variance), which `gpt_select_greedy` runs as one device-resident
pipeline: one new factor column over the pool per insertion instead of a refit.

Stated deviation.  The reference's inner regressor re-optimises the hyper-parameters from the initial kernel at EVERY
insertion (sklearn's default optimiser, no restarts).  This class holds them fixed during the selection:
  selection_theta="initial" (default)  the kernel as given — exactly the reference when the kernel's bounds are "fixed";
  selection_theta="fit_initial"        the package's hyper-parameter search, once, on the initial subset.
The final fit on the selected subset is the parent's, optimiser and restarts included, as the reference's (:68)."""
from __future__ import annotations

import numpy as np

from . import _lib
from .gaussian_process import GaussianProcess as _ExactGaussianProcess, kernel_hyperparameters, kernel_type

_SELECTION_THETA = ("initial", "fit_initial")


class ActiveLearningGaussianProcess(_ExactGaussianProcess):
    def __init__(self, kernel, alpha=1e-10, n_restarts_optimizer=5, n_samples_max=20000, optimizer="fmin_l_bfgs_b", device=0,
                 verbose=True, dtype="float64", selection_theta="initial", **parent_options):
        """(kernel, alpha, n_restarts_optimizer, n_samples_max) as the reference's (:16-20); `optimizer`, `device`,
        `verbose`, `dtype` as the parent's, and the parent's other keywords (`matern_derivatives`, `n_targets`, `devices`)
        are passed on to it (with `devices` the selection runs on devices[0]); `selection_theta`: the hyper-parameters
        the selection runs with (module docstring).  After a fit that selected: `selected_indices_` (rows of the X passed to fit, in insertion order: the
        initial subset, then the chosen points) and `selection_variance_` (the posterior variance, white noise included, of
        each chosen point when it was chosen — the square of the std the reference maximises); None otherwise."""
        if selection_theta not in _SELECTION_THETA:
            raise ValueError(f"selection_theta must be one of {_SELECTION_THETA}, got {selection_theta!r}")
        n_samples_max = int(n_samples_max)
        if n_samples_max < 1:
            raise ValueError("n_samples_max must be >= 1")
        super().__init__(kernel, alpha=alpha, optimizer=optimizer, n_restarts_optimizer=n_restarts_optimizer, device=device,
                         verbose=verbose, dtype=dtype, **parent_options)
        self.n_samples_max = n_samples_max
        self.selection_theta = selection_theta
        self.selected_indices_ = None
        self.selection_variance_ = None

    def fit(self, X, Y):
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]
        self.selected_indices_ = None
        self.selection_variance_ = None
        keep = np.flatnonzero(~np.isnan(Y).any(axis=1))          # the parent's NaN-row filter, before the selection
        if X.ndim != 2 or X.shape[0] <= self.n_samples_max or keep.size <= self.n_samples_max:
            return super().fit(X, Y)
        if X.shape[1] > _lib.MAX_D:
            raise ValueError(f"X has {X.shape[1]} features: this GPU path supports input dimension D = 1 .. {_lib.MAX_D} only")
        pool, targets = X[keep], Y[keep]
        if self.verbose:
            print("Starting Active Learning")
        n_initial = int(0.1 * self.n_samples_max)                # (:28)
        initial = np.random.choice(range(pool.shape[0]), size=n_initial, replace=False)     # (:31), numpy's global stream
        c, ls, noise = self._selection_hyperparameters(pool[initial], targets[initial])
        selected, selvar, _ = _lib.select_greedy(pool, ls, c, noise, self.alpha, self.n_samples_max, initial=initial,
                                                 kernel_type=kernel_type(self._kernel_in), device=self.device, residual=False)
        super().fit(pool[selected], targets[selected])           # the reference's row order: initial points, then insertions
        self.n_samples = self.n_samples_max                      # (:65)
        self.selected_indices_ = keep[selected]
        self.selection_variance_ = selvar
        return self

    def _selection_hyperparameters(self, X0, Y0):
        if self.selection_theta == "initial" or X0.shape[0] == 0:
            return kernel_hyperparameters(self._kernel_in)
        gp0 = _ExactGaussianProcess(self._kernel_in, alpha=self.alpha, optimizer=self.optimizer,
                                    n_restarts_optimizer=self.n_restarts_optimizer, device=self.device, verbose=False)
        gp0.fit(X0, Y0)
        return gp0._c, gp0._ls, gp0._noise


GaussianProcess = ActiveLearningGaussianProcess        # `from ...models.gaussian_process_al import GaussianProcess` ports as is
