"""The point-cloud surface SVGP: drop-in for the reference's plain StocasticVariationalGaussianProcess
(policy_transportation/models/torch/stocastic_variational_gaussian_process.py:15-111), the model that
sensors/surface_pointcloud_detector.py and example/3D/torch/fit_point_could.py fit to a camera point cloud.

It is not the transport model of svgp_exact.py: the RBF length-scale is per task, the whitened variational mean starts at
zero, and prediction is the variational predictive itself (`self.gp(x)`), with no conversion to pseudo-points.  Training
(`gpt_svgp_surface_train`) and prediction (`gpt_svgp_surface_predict`) are fp64 HIP; each task's Z x Z work (blocked
Cholesky and inverse, MFMA GEMMs) is spread over the whole GPU.

Deviations from the reference, by design:
  * fp64 throughout, where the reference trains and predicts in float32;
  * numpy's global RNG draws the inducing points (as the reference does, :19-20) and also the minibatch schedule, where
    the reference shuffles with torch's DataLoader;
  * the variational mean starts at exactly m = 0, where gpytorch's CholeskyVariationalDistribution adds 1e-3 noise;
  * parity with gpytorch is unpinned (gpytorch is not available): the objective is this repository's reading of its
    defaults (whitened VariationalStrategy, jitter 1e-4, MultitaskGaussianLikelihood with per-task and global noise);
  * `mean_fun` and `variance_fun`, the reference's torch-autograd helpers, are not mirrored."""
import numpy as np

from . import _lib
from .svgp_exact import svgp_schedule


class StocasticVariationalGaussianProcess:
    """SVGP of a point cloud: X (N,D) -> Y (N,T), `num_inducing` inducing points drawn from X with replacement."""

    def __init__(self, X, Y, num_inducing=100, device=0):
        self.X = np.asarray(X, dtype=np.float64)
        self.Y = np.asarray(Y, dtype=np.float64)
        if self.X.ndim != 2 or self.Y.ndim != 2 or len(self.X) != len(self.Y):
            raise ValueError(f"X (N,D) and Y (N,T) expected, got {self.X.shape} and {self.Y.shape}")
        (N, D), T = self.X.shape, self.Y.shape[1]
        if not 1 <= num_inducing <= _lib.SURFACE_MAX_INDUCING:
            raise ValueError(f"num_inducing must be 1 .. {_lib.SURFACE_MAX_INDUCING}, got {num_inducing}")
        if not 1 <= T <= _lib.SURFACE_MAX_TASKS:
            raise ValueError(f"Y must have 1 .. {_lib.SURFACE_MAX_TASKS} columns (tasks), got {T}")
        if not 1 <= D <= _lib.MAX_D:
            raise ValueError(f"X must have 1 .. {_lib.MAX_D} columns, got {D}")
        self.num_inducing = int(num_inducing)
        self.device = device
        sample_index = np.random.choice(np.arange(N), self.num_inducing)       # :19-20
        Zn = self.num_inducing
        self.variational_params_ = {"Z": self.X[sample_index].copy(), "m": np.zeros((T, Zn)), "C": np.tile(np.eye(Zn), (T, 1, 1)),
                                    "raw_ls": np.zeros((T, D)), "raw_os": np.zeros(T), "raw_noise": np.zeros(T + 1)}
        self.loss_history_ = np.zeros(0)

    def fit(self, num_epochs=10, lr=0.01, batch_size=10):
        """Adam (lr, betas 0.9 / 0.999) on the negative ELBO, `num_epochs` shuffled passes in minibatches (:68-89)."""
        if num_epochs < 1:
            raise ValueError(f"num_epochs must be >= 1, got {num_epochs}")
        if not 1 <= batch_size <= _lib.SURFACE_MAX_BATCH:
            raise ValueError(f"batch_size must be 1 .. {_lib.SURFACE_MAX_BATCH}, got {batch_size}")
        order, bb = svgp_schedule(len(self.X), num_epochs, batch_size)
        params = dict(self.variational_params_)
        trace = _lib.svgp_surface_train(self.X, self.Y, params, order, bb, lr=lr, device=self.device)
        self.variational_params_ = params
        self.loss_history_ = np.concatenate([self.loss_history_, trace])
        return self

    def _query(self, x):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.X.shape[1]:
            raise ValueError(f"queries must be (M, {self.X.shape[1]}), got {x.shape}")
        return x

    def predict(self, x, return_std=False):
        """Mean (M,T) of the latent f, and its std (M,T) when asked (:95-103)."""
        mean, var, _ = _lib.svgp_surface_predict(self.variational_params_, self._query(x), var=return_std, device=self.device)
        if return_std:
            return mean, np.sqrt(np.maximum(var, 0.0))
        return mean

    def derivative(self, x):
        """J (M,T,D) = d mean / d x: the layout of the reference's jacobian(mean_fun, x).transpose(1,0,2) (:105-111)."""
        _, _, J = _lib.svgp_surface_predict(self.variational_params_, self._query(x), J=True, device=self.device)
        return J
