"""GaussianProcess — host-side mirror of the reference regressor
(policy_transportation/models/gaussian_process.py:16-126) running on an MI355X through
libgpt_hip.  Same constructor, methods, shapes and quirks; the numerics (Gram, Cholesky,
alpha, posterior mean / variance / Jacobian / Jacobian variance / d var/dx) are HIP kernels.
scikit-learn kernel objects are accepted as hyper-parameter containers only."""
from __future__ import annotations

import copy

import numpy as np

from . import _lib

_PARAM_C = "k1__k1__constant_value"
_PARAM_LS = "k1__k2__length_scale"
_PARAM_NOISE = "k2__noise_level"


def kernel_hyperparameters(kernel):
    """(constant_value, length_scale array, noise_level) of a `ConstantKernel * RBF + WhiteKernel`
    object — the parameter names the reference hard-codes (gaussian_process.py:39-41, 49)."""
    try:
        p = kernel.get_params()
        c, ls, noise = p[_PARAM_C], p[_PARAM_LS], p[_PARAM_NOISE]
    except (AttributeError, KeyError) as e:
        raise ValueError("kernel must be ConstantKernel * RBF + WhiteKernel (as the reference's parameter "
                         "names k1__k1__constant_value / k1__k2__length_scale / k2__noise_level require)") from e
    return float(c), np.atleast_1d(np.asarray(ls, dtype=np.float64)), float(noise)


def kernel_type(kernel):
    """GPT_KERNEL_* code of the stationary factor: RBF, or Matern with nu in {0.5, 1.5, 2.5, inf}."""
    k = kernel.get_params().get("k1__k2", None)
    name = type(k).__name__
    if name == "RBF":
        return 0
    if name == "Matern":
        nu = float(k.nu)
        codes = {0.5: 1, 1.5: 2, 2.5: 3, float("inf"): 0}
        if nu in codes:
            return codes[nu]
        raise NotImplementedError(f"Matern(nu={nu}) is not on the GPU path (nu must be 0.5, 1.5, 2.5 or inf)")
    raise NotImplementedError(f"only RBF and Matern kernels run on the GPU path, got {name}")


class _FittedView:
    """Stands in for the reference's `self.gp` (the sklearn estimator): the fitted attributes
    outside callers read, fetched from the device on first access."""

    def __init__(self, owner):
        self._o = owner
        self._L = None
        self._alpha_ = None
        self.alpha = owner.alpha
        self.kernel = owner._kernel_in
        self.kernel_ = None
        self.X_train_ = None
        self.y_train_ = None
        self._lml = None

    @property
    def alpha_(self):
        if self._alpha_ is None:
            self._alpha_ = self._o._handle.export(want_L=False)[1]
        return self._alpha_

    @property
    def log_marginal_likelihood_value_(self):
        """LML of the fitted theta (sklearn/_gpr.py:335-341), evaluated on the device on first access."""
        if self._lml is None:
            self._lml = self._o._handle.lml()
        return self._lml

    @property
    def L_(self):
        if self._L is None:
            self._L = self._o._handle.export(want_alpha=False)[0]
        return self._L


class GaussianProcess:
    def __init__(self, kernel, alpha=1e-10, optimizer="fmin_l_bfgs_b", n_restarts_optimizer=5, n_targets=None,
                 device=0, verbose=True, dtype="float64", devices=None, matern_derivatives=False):
        """Arguments as the reference's (:17-23); `device`, `devices`, `verbose` and `dtype` are additions.  dtype="float32"
        keeps the fp64 factorisation and runs the prediction kernels in fp32 (outputs float32; return_cov / samples need
        float64): twice the fp64 rate, ~1e-4 of the output scale.  devices=[0, 1, ...] (default: the one `device`): the fit
        and the hyper-parameter search run on devices[0], the fitted model is copied to the others and predict / derivative
        / derivative_of_variance shard their rows over all of them (device_group.py) — same results, same call.
        matern_derivatives=True: derivative / derivative_of_variance / posterior / prefetch_posterior of a Matern(nu=1.5 or
        2.5) model return the analytic derivatives of its posterior (the reference multiplies the Matern k* by the RBF
        coefficient instead, which this path does not reproduce).  Default False: those calls raise NotImplementedError, as
        the reference's numbers or a refusal are the drop-in's rule.  No effect on RBF models; nu=0.5 is refused either way."""
        if isinstance(optimizer, str) and optimizer == "device_bfgs":
            raise ValueError("optimizer='device_bfgs' is the on-device search of a batch of small models (n <= 128 points each): use "
                             "GaussianProcessBatch or GaussianProcessTransportationBatch.  GaussianProcess takes 'fmin_l_bfgs_b', a "
                             "callable or None")
        self._kernel_in = kernel
        self.kernel = kernel
        self.alpha = alpha
        self.optimizer = optimizer
        self.n_restarts_optimizer = n_restarts_optimizer if optimizer is not None else 0
        self.n_targets = n_targets
        self.devices = [int(d) for d in devices] if devices is not None else None
        if self.devices is not None and not self.devices:
            raise ValueError("devices must name at least one GPU")
        self.device = self.devices[0] if self.devices else device
        self.verbose = verbose
        self.matern_derivatives = bool(matern_derivatives)
        if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        self._dtype = _lib.GPT_F32 if np.dtype(dtype) == np.dtype(np.float32) else _lib.GPT_F64
        self._handle = None
        self._K_inv = None
        self.gp = _FittedView(self)

    # ------------------------------------------------------------------ fit
    def fit(self, X, Y):
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]
        self.X = X
        self.Y = Y
        self._memo = None
        self.n_features = np.shape(X)[1]
        self.n_samples = np.shape(X)[0]          # pre-filter count, as the reference (:29)
        self.n_outputs = np.shape(Y)[1]
        mask = np.isnan(Y).any(axis=1)           # (:33-35)
        self.X = X[~mask]
        self.Y = Y[~mask]
        if self.n_targets is not None and self.n_outputs != self.n_targets:   # sklearn/_gpr.py:265-269
            raise ValueError(f"The number of targets seen in `y` is different from the parameter `n_targets`. "
                             f"Got {self.n_outputs} != {self.n_targets}.")
        c, ls, noise = kernel_hyperparameters(self._kernel_in)
        self._ktype = kernel_type(self._kernel_in)
        lml = None
        if self.optimizer is not None:
            from .hyperopt import optimize_hyperparameters
            c, ls, noise, lml = optimize_hyperparameters(self, c, ls, noise)
        if self._handle is None:
            self._handle = self._new_handle()
        self._handle.set_dtype(self._dtype)
        self._handle.set_matern_derivatives(self.matern_derivatives)
        self._handle.fit(self.X, self.Y, ls, c, noise, self.alpha, self._ktype)
        self._K_inv = None
        self._fit_token = object()               # what was drawn from an earlier fit knows that it is not this one (posterior_functions.py)
        # fitted kernel object with the reference's attribute protocol (:38-41)
        fitted = copy.deepcopy(self._kernel_in)
        keep_array = np.iterable(self._kernel_in.get_params()[_PARAM_LS])
        fitted.set_params(**{_PARAM_C: c, _PARAM_LS: (ls.copy() if keep_array else float(ls[0])), _PARAM_NOISE: noise})
        self.kernel = fitted
        self.gp = _FittedView(self)
        self.gp._lml = lml
        self.gp.kernel_ = fitted
        self.gp.X_train_ = self.X
        self.gp.y_train_ = self.Y
        self.kernel_params_ = [fitted.get_params()[_PARAM_LS], fitted.get_params()["k1"]]
        self.noise_var_ = self.alpha + noise
        self.prior_var = c
        self._c, self._ls, self._noise = c, ls, noise
        if self.verbose:
            print("lenghtscales", fitted.get_params()[_PARAM_LS])
        return self

    def _new_handle(self):
        """One handle on `device`, or — devices=[a, b, ...] — the group that fits on the first and predicts on all."""
        if self.devices is not None and len(self.devices) > 1:
            from .device_group import DeviceGroup
            return DeviceGroup(self.devices)
        return _lib.Handle(self.device)

    @property
    def K_inv(self):
        """(c*RBF + noise_var_*I)^-1 as the reference caches it (:42-43).  Only reference-internal
        code reads it; here it is assembled lazily from the device factor W = L^-1 (K^-1 = W^T W)."""
        if self._K_inv is None:
            W = self._handle.export_inverse_factor()
            self._K_inv = W.T @ W
        return self._K_inv

    def _require_derivatives(self, what):
        """RBF: the reference's formulas.  Matern 3/2 and 5/2: the analytic derivatives of the posterior, opt-in."""
        if self._ktype == 0:
            return
        if self._ktype == 1:
            raise NotImplementedError(f"{what}(): Matern(nu=0.5) is not differentiable at the training points (its derivative "
                                      "has infinite prior variance); derivatives need RBF or Matern with nu=1.5 / 2.5")
        if not self.matern_derivatives:
            raise NotImplementedError(f"{what}() implements the RBF formulas of the reference (gaussian_process.py:63-126); "
                                      "the reference silently applies them to any kernel, this path refuses.  "
                                      "GaussianProcess(..., matern_derivatives=True) gives the analytic derivatives of the "
                                      "Matern posterior instead (not the reference's numbers)")

    def _require_fit(self):
        if self._handle is None:
            raise RuntimeError("GaussianProcess is not fitted")

    # ------------------------------------------------------------------ predict
    def predict(self, x, return_std=False, return_cov=False):
        """(:46-55)  mean (M,O); with return_std also `std - sqrt(noise_level)` tiled over outputs."""
        self._require_fit()
        if return_std and return_cov:
            raise RuntimeError("At most one of return_std or return_cov can be requested.")
        if return_cov:                                  # sklearn/_gpr.py:458-470
            mean, cov = self._handle.predict_cov(x)
            if self.n_outputs == 1:
                return mean[:, 0], cov
            return mean, np.repeat(cov[:, :, None], self.n_outputs, axis=2)
        out = self._memo_lookup(x) or self._handle.predict_all(x, mean=True, var=bool(return_std))
        mean = out["mean"]
        if self.n_outputs == 1:
            mean = mean[:, 0]                       # sklearn squeezes single-target output (_gpr.py:449-451)
        if not return_std:
            return mean
        std = np.sqrt(out["var"])
        if self.n_outputs > 1:
            std = np.repeat(std[:, None], self.n_outputs, axis=1)   # _gpr.py:488
        return mean, std - np.sqrt(self._noise)     # reference quirk (:49)

    def samples(self, x):
        """(:57-60)  10 joint posterior draws per output, shape (10, M, O).  Mean and covariance come from the
        GPU; the draws follow sklearn's sample_y (sklearn/_gpr.py:498-535: RandomState(0),
        multivariate_normal per target) on the host."""
        self._require_fit()
        mean, cov = self._handle.predict_cov(x)
        rng = np.random.RandomState(0)
        per_target = [rng.multivariate_normal(mean[:, t], cov, 10).T[:, np.newaxis] for t in range(self.n_outputs)]
        y_samples = np.hstack(per_target)               # (M, O, 10)
        return np.transpose(y_samples, (2, 0, 1))

    # ------------------------------------------------------------------ derivatives
    def derivative(self, x, return_var=False):
        """(:63-102)  J (M,O,D) = d mean_o / d x_d; with return_var also its variance, tiled over outputs."""
        self._require_fit()
        self._require_derivatives("derivative")
        out = self._memo_lookup(x) or self._handle.predict_all(x, J=True, Jvar=bool(return_var))
        if not return_var:
            return out["J"]
        Sigma = np.repeat(out["Jvar"][:, None, :], self.n_outputs, axis=1)
        return out["J"], Sigma

    def derivative_of_variance(self, x):
        """(:104-126)  (D, M) array of d var / d x_d."""
        self._require_fit()
        self._require_derivatives("derivative_of_variance")
        return self._handle.predict_all(x, dvar=True)["dvar"]

    # ------------------------------------------------------------------ inverse of the displacement map
    def invert_displacement(self, y, x0=None, rtol=1e-10, max_passes=64, return_info=False):
        """The z (M,D) with z + predict(z) = y: the map x -> x + predict(x) that PolicyTransportation.transport applies
        after its affine part, inverted by damped Newton on the device, every query in one wave of one launch
        (_lib.Handle.inverse_map; the reference only approximates this with a second transport fitted backwards,
        example/2D/surface_generalization_heteroschedastic _inverse_mapping.py:88-127).  x0 (M,D): start points (default y).
        A query stops when |z + predict(z) - y| <= rtol (1 + |y|) or after max_passes evaluations of the model.
        With return_info also a dict: status (M,) (_lib.INV_CONVERGED / INV_MAX_PASSES / INV_SINGULAR / INV_STALLED), passes
        (M,), residual (M,), det (M,) = det(I + derivative(z)) — not positive where the map folds and the solution is one
        of several.  Needs n_outputs == n_features <= 3, float64, and for a Matern model matern_derivatives=True.  With
        devices=[...] it runs on the device that holds the fit."""
        self._require_fit()
        if self.n_outputs != self.n_features or self.n_features > 3:
            raise NotImplementedError(f"invert_displacement(): the inverse needs a map of a space onto itself with at most 3 "
                                      f"dimensions (this model: {self.n_features} features, {self.n_outputs} outputs)")
        if self._dtype != _lib.GPT_F64:
            raise NotImplementedError("invert_displacement(): float64 models only (this one was built with dtype='float32')")
        self._require_derivatives("invert_displacement")
        if not float(rtol) > 0.0:
            raise ValueError("invert_displacement(): rtol must be > 0")
        if int(max_passes) < 1:
            raise ValueError("invert_displacement(): max_passes must be >= 1")
        y = _lib.as_f64(y, 2, "y")
        if y.shape[1] != self.n_features:
            raise ValueError(f"y has {y.shape[1]} columns, the model {self.n_features} features")
        if x0 is not None:
            x0 = _lib.as_f64(x0, 2, "x0")
            if x0.shape != y.shape:
                raise ValueError(f"x0 has shape {x0.shape}, y {y.shape}")
        if y.shape[0] >= 2 ** 31:
            raise ValueError("invert_displacement(): fewer than 2^31 points per call")
        z, info = self._handle.inverse_map(y, x0, rtol=rtol, max_passes=max_passes)
        return (z, info) if return_info else z

    # ------------------------------------------------------------------ the whole transport in one device call
    def transport_policy(self, x, rotation, scale, source_centroid, target_centroid, jacobian=None, vel=None, ori=None,
                         return_posterior=False):
        """Phi(x) = gamma(x) + predict(gamma(x)), gamma(x) = scale * rotation (x - source_centroid) + target_centroid, with the
        velocities `vel` (M,D) and orientations `ori` (M,4; w,x,y,z) pushed through its Jacobian — the affine part, the
        posterior and the algebra of PolicyTransportation.transport / transport_velocity / transport_orientation in one
        call on the device (_lib.Handle.transport_policy).  `jacobian`: the Jacobian of gamma (default `rotation`, unscaled: the
        reference's quirk).  Returns a dict: pos (M,D), pos_rot = gamma(x), std (as predict returns it), and with vel: vel,
        vel_var (M,D) (as transport_velocity returns them), det_vel (M,); with ori: ori (M,4), ori_gap (M,) (0 where the closest
        rotation is not unique) — both None unless D = 3 — and det_ori (M,) = det of the Jacobian at the UN-rotated x (the
        reference's choice).
        return_posterior: also post_mean, post_J, post_Jvar at gamma(x) and post_J_ori at x.  Needs n_outputs == n_features <= 3,
        float64, and for a Matern model matern_derivatives=True.  With devices=[...] it runs on the device that holds the fit."""
        self._require_fit()
        if self.n_outputs != self.n_features or self.n_features > 3:
            raise NotImplementedError(f"transport_policy(): the transport needs a map of a space onto itself with at most 3 "
                                      f"dimensions (this model: {self.n_features} features, {self.n_outputs} outputs)")
        if self._dtype != _lib.GPT_F64:
            raise NotImplementedError("transport_policy(): float64 models only (this one was built with dtype='float32')")
        self._require_derivatives("transport_policy")
        D = self.n_features
        want_ori = ori is not None
        if want_ori and D != 3:                  # no quaternion of a 1-D or 2-D Jacobian: its determinant alone ("ori": None)
            ori = None
        names = ["pos_rot", "pos_out", "var"]
        if vel is not None:
            names += ["vel_out", "vel_var", "det_vel"]
        if want_ori:
            names += ["det_ori"]
        if ori is not None:
            names += ["ori_out", "ori_gap"]
        if return_posterior:
            names += ["post_mean", "post_J", "post_Jvar", "post_J_ori"]
        out = self._handle.transport_policy(x, rotation, source_centroid, target_centroid, scale=scale, R_jac=jacobian, vel=vel, ori=ori,
                                            outputs=names)
        std = np.sqrt(out["var"])
        if self.n_outputs > 1:
            std = np.repeat(std[:, None], self.n_outputs, axis=1)
        res = {"pos": out["pos_out"], "pos_rot": out["pos_rot"], "std": std - np.sqrt(self._noise)}
        if vel is not None:
            res.update(vel=out["vel_out"], vel_var=np.repeat(out["vel_var"][:, None], self.n_outputs, axis=1), det_vel=out["det_vel"])
        if want_ori:
            res.update(ori=out.get("ori_out"), ori_gap=out.get("ori_gap"), det_ori=out["det_ori"])
        if return_posterior:
            res.update({k: out[k] for k in ("post_mean", "post_J", "post_Jvar", "post_J_ori")})
        return res

    # ------------------------------------------------------------------ the transported policy at target-space points
    def _require_self_map(self, what, role):
        if self.n_outputs != self.n_features or self.n_features > 3:
            raise NotImplementedError(f"{what}(): the {role} must be a model of a space onto itself with at most 3 dimensions "
                                      f"(this model: {self.n_features} features, {self.n_outputs} outputs)")
        if self._dtype != _lib.GPT_F64:
            raise NotImplementedError(f"{what}(): float64 models only (the {role} was built with dtype='float32')")

    def pullback_policy(self, dynamics, y, rotation, scale, source_centroid, target_centroid, jacobian=None, x0=None, rtol=1e-10,
                        max_passes=64, variances=False, return_posterior=False):
        """The transported policy at the target-space points y (M,D): with this model psi the displacement of the transport
        Phi(x) = gamma(x) + predict(gamma(x)), gamma(x) = scale * rotation (x - source_centroid) + target_centroid, and `dynamics`
        a second fitted GaussianProcess f of the source scene (any kernel, Matern(nu=0.5) included: it is only evaluated),
            x = Phi^-1(y),   vel = J_Phi(x) dynamics.predict(x)
        — the inverse (damped Newton as invert_displacement, started at gamma(x0) when x0 (M,D), a guess of the preimages, is
        given), the dynamics mean and the push-forward in one launch on the device (_lib.Handle.pullback_policy), instead of
        the reference's second GP fitted on the moved demonstration (example/2D/surface_generalization.py:81-88).  `jacobian`:
        the Jacobian of gamma (default `rotation`, unscaled: the reference's quirk).  Returns a dict: x (M,D), vel (M,D), f (M,D)
        = dynamics.predict(x), status, passes, residual, det (M,) as invert_displacement's info — a point that did not converge
        has every value at the z it reached and says so in status.  variances=True adds std_dyn (M,D) = the std
        dynamics.predict(x, return_std=True) returns, map_std (M,D) = this model's at gamma(x), vel_var_dyn (M,D) = std_dyn^2
        times the row sums of J_Phi^2, and vel_var_map (M,D) = the variance transport_velocity returns for (x, f);
        variances="vel" leaves map_std out (the variance of vel does not need it, and without it the map's variance launch has
        three columns per point instead of four).
        return_posterior: also post_z (M,D) = gamma(x), post_A (M,D,D) = I + derivative(post_z) and, with variances, post_Jvar
        (M,D).  Both models need n_outputs == n_features <= 3 (the same), float64; this one, if Matern, matern_derivatives=True.
        With devices=[...] the call runs on the device that holds the fit; the dynamics must hold its fit on the same device."""
        self._require_fit()
        self._require_self_map("pullback_policy", "map")
        self._require_derivatives("pullback_policy")
        if not isinstance(dynamics, GaussianProcess):
            raise NotImplementedError(f"pullback_policy(): the dynamics ({type(dynamics).__name__}) must be a fitted GaussianProcess")
        if dynamics is self:
            raise ValueError("pullback_policy(): the map and the dynamics are the same object; they are two models")
        dynamics._require_fit()
        dynamics._require_self_map("pullback_policy", "dynamics")
        if dynamics.n_features != self.n_features:
            raise ValueError(f"pullback_policy(): the map has {self.n_features} features, the dynamics {dynamics.n_features}")
        if dynamics.device != self.device:
            raise ValueError(f"pullback_policy(): the map holds its fit on device {self.device}, the dynamics on {dynamics.device}")
        if not float(rtol) > 0.0:
            raise ValueError("pullback_policy(): rtol must be > 0")
        if int(max_passes) < 1:
            raise ValueError("pullback_policy(): max_passes must be >= 1")
        y = _lib.as_f64(y, 2, "y")
        if y.shape[1] != self.n_features:
            raise ValueError(f"y has {y.shape[1]} columns, the model {self.n_features} features")
        if x0 is not None:
            x0 = _lib.as_f64(x0, 2, "x0")
            if x0.shape != y.shape:
                raise ValueError(f"x0 has shape {x0.shape}, y {y.shape}")
        if y.shape[0] >= 2 ** 31:
            raise ValueError("pullback_policy(): fewer than 2^31 points per call")
        names = ["x", "vel", "f", "det", "residual", "passes", "status"]
        if variances not in (False, True, "vel"):
            raise ValueError("pullback_policy(): variances is False, True or 'vel'")
        if variances:
            names += ["var_dyn", "vel_var_map", "vel_var_dyn"] + (["map_var"] if variances is True else [])
        if return_posterior:
            names += ["post_z", "post_A"] + (["post_Jvar"] if variances else [])
        dyn_handle = getattr(dynamics._handle, "primary", dynamics._handle)
        out = self._handle.pullback_policy(dyn_handle, y, rotation, source_centroid, target_centroid, scale=scale, R_jac=jacobian, x0=x0,
                                           rtol=rtol, max_passes=max_passes, std_offset=np.sqrt(dynamics._noise), outputs=names)
        res = {k: out[k] for k in ("x", "vel", "f", "status", "passes", "residual", "det")}
        if variances:
            D = self.n_outputs
            tile = lambda v: np.repeat(v[:, None], D, axis=1) if D > 1 else v
            res.update(std_dyn=tile(np.sqrt(out["var_dyn"])) - np.sqrt(dynamics._noise),
                       vel_var_dyn=out["vel_var_dyn"], vel_var_map=np.repeat(out["vel_var_map"][:, None], D, axis=1))
            if variances is True:
                res.update(map_std=tile(np.sqrt(out["map_var"])) - np.sqrt(self._noise))
        if return_posterior:
            res.update({k: out[k] for k in names if k.startswith("post_")})
        return res

    @staticmethod
    def _check_chain(what, maps, dynamics, affine, k_min):
        """What pullback_chain() and rollout_chain() refuse of their models before anything reaches a device: the number of maps
        (k_min .. CHAIN_MAX) and of affine parts, kinds, fits, dimensions, dtypes, derivatives of the maps, one object twice, devices.
        The model the others are compared with is the last map (without maps: the dynamics).  Returns the affine parts as a list."""
        if not k_min <= len(maps) <= _lib.CHAIN_MAX:
            raise ValueError(f"{what}(): {k_min} .. {_lib.CHAIN_MAX} maps, got {len(maps)}")
        affine = list(affine)
        if len(affine) != len(maps):
            raise ValueError(f"{what}(): {len(maps)} maps, {len(affine)} affine parts")
        if not isinstance(dynamics, GaussianProcess):
            raise NotImplementedError(f"{what}(): the dynamics ({type(dynamics).__name__}) must be a fitted GaussianProcess")
        for k, g in enumerate(maps):
            if not isinstance(g, GaussianProcess):
                raise NotImplementedError(f"{what}(): the map of stage {k} ({type(g).__name__}) must be a fitted GaussianProcess")
            g._require_fit()
            g._require_self_map(what, f"map of stage {k}")
            g._require_derivatives(what)
        dynamics._require_fit()
        dynamics._require_self_map(what, "dynamics")
        models = maps + [dynamics]
        if len({id(g) for g in models}) != len(models):
            raise ValueError(f"{what}(): one object twice among the maps and the dynamics; each is a model of its own")
        last = models[-2] if maps else dynamics
        for k, g in enumerate(models):
            who = "the dynamics" if g is dynamics else f"the map of stage {k}"
            if g.n_features != last.n_features:
                raise ValueError(f"{what}(): the last map has {last.n_features} features, {who} {g.n_features}")
            if g.device != last.device:
                raise ValueError(f"{what}(): the last map holds its fit on device {last.device}, {who} on {g.device}")
        return affine

    def _check_chain_points(self, what, y, x0, rtol, max_passes, name):
        """The solver's arguments and the points (M,D) with their optional guesses, as float64 arrays."""
        if not float(rtol) > 0.0:
            raise ValueError(f"{what}(): rtol must be > 0")
        if int(max_passes) < 1:
            raise ValueError(f"{what}(): max_passes must be >= 1")
        y = _lib.as_f64(y, 2, name)
        if y.shape[1] != self.n_features:
            raise ValueError(f"{name} has {y.shape[1]} columns, the model {self.n_features} features")
        if x0 is not None:
            x0 = _lib.as_f64(x0, 2, "x0")
            if x0.shape != y.shape:
                raise ValueError(f"x0 has shape {x0.shape}, {name} {y.shape}")
        if y.shape[0] >= 2 ** 31:
            raise ValueError(f"{what}(): fewer than 2^31 points per call")
        return y, x0

    def pullback_chain(self, inner, dynamics, y, affine, x0=None, rtol=1e-10, max_passes=64, variances=False, outputs=None):
        """The transported policy at the target-space points y (M,D) through a CHAIN of transports Phi = Phi_{K-1} o ... o Phi_0,
        this model the displacement psi_{K-1} of the LAST one and `inner` the GaussianProcess models psi_0 .. psi_{K-2} of the
        ones applied before it (K <= 4):  x = Phi^-1(y),  vel = J_Phi(x) dynamics.predict(x), the K inverses, the dynamics mean and
        the push-forward in one launch on the device (_lib.Handle.pullback_chain).  `affine`: K tuples (rotation, scale,
        source_centroid, target_centroid, jacobian), stage 0 first, jacobian None for the rotation.  x0 (M,D): guesses of the
        SOURCE-space preimages; they are pushed forward through the means to give every stage its start.  Returns a dict: x,
        vel, f (M,D), status (M,) = the status of the first stage in solve order (the last stage first) that did not converge,
        and per stage, stage-major (K,M,...): stage_x, stage_z, stage_A, stage_status, stage_passes, stage_residual, stage_det — a
        stage that does not converge hands on the point it reached.  variances=True adds var_dyn (M,), vel_var_dyn (M,D),
        vel_var_map (M,D) (each map's Jacobian variance pushed through the maps after it, summed), stage_Jvar (K,M,D) and
        stage_map_var (K,M); variances="vel" leaves stage_map_var out.  `outputs`: instead of all that, just these names of
        _lib.CHAIN_OUTPUTS (vel and status always come) — every array left out is one copy from the device less, which at a
        handful of points is most of the call.  Every model needs n_outputs == n_features <= 3 (the
        same), float64, a fit on one device; the maps, if Matern, matern_derivatives=True."""
        maps = list(inner) + [self]
        affine = self._check_chain("pullback_chain", maps, dynamics, affine, 1)
        y, x0 = self._check_chain_points("pullback_chain", y, x0, rtol, max_passes, "y")
        if variances not in (False, True, "vel"):
            raise ValueError("pullback_chain(): variances is False, True or 'vel'")
        names = ["x", "vel", "f", "status", "stage_x", "stage_z", "stage_A", "stage_status", "stage_passes", "stage_residual", "stage_det"]
        if variances:
            names += ["var_dyn", "vel_var_map", "vel_var_dyn", "stage_Jvar"] + (["stage_map_var"] if variances is True else [])
        if outputs is not None:
            names = list(outputs)
        primary = lambda g: getattr(g._handle, "primary", g._handle)
        stages = [(primary(g), rot, src, dst, scale, jac) for g, (rot, scale, src, dst, jac) in zip(maps, affine)]
        return primary(self).pullback_chain(stages, primary(dynamics), y, x0=x0, rtol=rtol, max_passes=max_passes,
                                            std_offset=np.sqrt(dynamics._noise), outputs=names)

    # ------------------------------------------------------------------ whole paths of the transported policy
    def rollout_chain(self, inner, dynamics, starts, n_steps, affine, dt=1.0, x0=None, rtol=1e-10, max_passes=64, outputs=("vel", "x"),
                      variance_gain=None):
        """The paths the transported policy of pullback_chain() drives from `starts` (M,D): n_steps explicit Euler steps
        y_{t+1} = y_t + dt * vel(y_t), the loop over the steps on the device in one call (_lib.Handle.rollout_policy) instead of one
        pullback_chain() per step; this model is the LAST map, `inner` the ones before it, `affine` as pullback_chain's.  Step t
        evaluates exactly what pullback_chain() returns for the point y_t with x0 = the x of step t - 1 (at t = 0: `x0`, guesses of
        the source-space preimages of the starts, or none).  dt: finite, not zero; negative integrates backwards.  A trajectory ends
        at the first step whose inverse does not converge or whose next point is not finite.  Returns a dict: path
        (M,n_steps+1,D) with row 0 the starts, steps_done (M,) the steps whose next point was recorded, status (M,) the
        _lib.INV_* of the last step evaluated, and — `outputs` — vel, x (M,n_steps,D); every row after a trajectory's end is NaN.
        variance_gain=None integrates the mean policy only.  A number >= 0 takes the variance-stabilised step instead, still in
        one device call (_lib.Handle.rollout_stabilised): with var and dvar the posterior variance of `dynamics` and its gradient at
        x_t, vel_t = push(f_t - variance_gain * (sqrt(var_t) - sqrt(noise)) * dvar_t / |dvar_t|), pushed through the maps as f_t
        is (the reference's plot_traj_evolution with gain 1; dvar / |dvar| is 0 where dvar is exactly 0).  The target-space path
        is then, to first order in dt, the image of the stabilised source-space path: the variance descended is the dynamics' own
        at the preimage, not that of a GP refitted on the moved demonstration.  `outputs` may then also name f, var, dvar.  The
        dynamics needs at most _lib.ROLLOUT_STAB_MAX_N training points and a kernel with derivatives."""
        maps = list(inner) + [self]
        affine = self._check_chain("rollout_chain", maps, dynamics, affine, 1)
        return self._rollout("rollout_chain", maps, affine, dynamics, starts, n_steps, dt, x0, rtol, max_passes, outputs, variance_gain)

    def rollout(self, starts, n_steps, dt=1.0, return_info=False, variance_gain=None):
        """This model as a dynamics rolling out itself: n_steps explicit Euler steps y_{t+1} = y_t + dt * predict(y_t) from every
        row of `starts` (M,D), the loop over the steps on the device (any of the four kernels: the model is only evaluated).
        Returns path (M,n_steps+1,D), row 0 the starts; with return_info also a dict: vel (M,n_steps,D) the means along the path,
        x (= the path's points), steps_done and status (M,).  A trajectory ends where its next point is not finite; the rows after
        that are NaN.  Needs n_outputs == n_features <= 3 and float64.
        variance_gain=None: that, untouched.  A number >= 0: the variance-stabilised step of the reference's plot_traj_evolution,
        y_{t+1} = y_t + dt * (predict(y_t) - variance_gain * std(y_t) * grad_var(y_t) / |grad_var(y_t)|), std as
        predict(return_std=True) and grad_var as derivative_of_variance (0 / 0 taken as 0), still one device call; the info dict
        then also holds f (the means), var (M,n_steps) and dvar (M,n_steps,D), and vel is the stabilised velocity.  One step
        (n_steps=1) from a grid of starts with variance_gain=2 is the field of the reference's plot_vector_field_minvar, in vel.
        The model then needs at most _lib.ROLLOUT_STAB_MAX_N training points and a kernel with derivatives."""
        self._check_chain("rollout", [], self, [], 0)
        names = ("vel", "x") + (("f", "var", "dvar") if variance_gain is not None else ())
        out = self._rollout("rollout", [], [], self, starts, n_steps, dt, None, 1e-10, 64, names if return_info else (), variance_gain)
        return (out["path"], {k: v for k, v in out.items() if k != "path"}) if return_info else out["path"]

    def _rollout(self, what, maps, affine, dynamics, starts, n_steps, dt, x0, rtol, max_passes, outputs, variance_gain=None):
        starts, x0 = self._check_chain_points(what, starts, x0, rtol, max_passes, "starts")
        if int(n_steps) != n_steps or int(n_steps) < 0:
            raise ValueError(f"{what}(): n_steps must be an integer >= 0, got {n_steps!r}")
        if not np.isfinite(float(dt)) or float(dt) == 0.0:
            raise ValueError(f"{what}(): dt must be finite and not zero, got {dt!r}")
        if starts.shape[0] * (int(n_steps) + 1) >= 2 ** 31:
            raise ValueError(f"{what}(): starts times (n_steps + 1), the rows of the paths, must stay below 2^31")
        primary = lambda g: getattr(g._handle, "primary", g._handle)
        stages = [(primary(g), rot, src, dst, scale, jac) for g, (rot, scale, src, dst, jac) in zip(maps, affine)]
        if variance_gain is None:
            return primary(self).rollout_policy(stages, primary(dynamics), starts, int(n_steps), dt=float(dt), x0=x0, rtol=rtol,
                                                max_passes=max_passes, outputs=outputs)
        if not np.isfinite(float(variance_gain)) or float(variance_gain) < 0.0:
            raise ValueError(f"{what}(): variance_gain must be finite and >= 0, got {variance_gain!r}")
        dynamics._require_derivatives(what)
        if len(dynamics.X) > _lib.ROLLOUT_STAB_MAX_N:
            raise ValueError(f"{what}(): the dynamics has {len(dynamics.X)} training points; the stabilised rollout takes at most "
                             f"{_lib.ROLLOUT_STAB_MAX_N} (larger models: predict and derivative_of_variance per step)")
        return primary(self).rollout_stabilised(stages, primary(dynamics), starts, int(n_steps), float(variance_gain),
                                                std_offset=np.sqrt(dynamics._noise), dt=float(dt), x0=x0, rtol=rtol,
                                                max_passes=max_passes, outputs=outputs)

    # ------------------------------------------------------------------ paths of functions drawn from the posterior
    def rollout_samples(self, starts, n_steps, n_samples=10, dt=1.0, nugget=None, random_state=0, normals=None, return_info=False):
        """Which paths does this model, as a dynamics, consider plausible from `starts` (M,D)?  n_samples paths per start, each the
        rollout y_{t+1} = y_t + dt * F(y_t) of ONE function F drawn from the posterior: the value drawn at step t is conditioned
        on what the same function was drawn to be at the path's own earlier points (the errors of a GP at neighbouring points are
        almost perfectly correlated; independent noise per step would understate the spread of a path by orders of magnitude).
        The loop over the steps, the covariance rows and the growing Cholesky factor run on the device in one call
        (_lib.Handle.rollout_sampled); any of the four kernels.  nugget: added to the diagonal of a path's covariance; None takes
        the noise level, which draws noisy values (the convention of predict(return_cov=True) and samples()); a small positive
        number draws the latent function.  normals (M,n_samples,n_steps,D): the standard normal numbers to use, else
        np.random.RandomState(random_state).standard_normal of that shape — sample j of start m does not depend on the other
        starts or samples.  Returns paths (M,n_samples,n_steps+1,D); with return_info also a dict: vel, x, f (M,S,n_steps,D), pvar,
        cvar (M,S,n_steps: the marginal and the conditional variance of a step's draw), steps_done, status (M,S; the _lib.INV_*
        values or _lib.ROLLOUT_DEGENERATE: the conditional variance fell to rounding level, which a nugget >= the noise level
        does not let happen); return_info="chol" adds chol (M,S,n_steps,n_steps), the factor of each path's covariance.  A path
        ends where its next point is not finite; the rows after that are NaN.  Zero normals give rollout().  Needs
        n_outputs == n_features <= 3, float64, at most _lib.ROLLOUT_STAB_MAX_N training points and _lib.ROLLOUT_SAMPLED_MAX_T
        steps (beyond: the host loop of examples/sampled_rollout_2d.py --host)."""
        self._check_chain("rollout_samples", [], self, [], 0)
        out = self._rollout_samples("rollout_samples", [], [], self, starts, n_steps, n_samples, dt, nugget, random_state, normals, None,
                                    1e-10, 64, return_info)
        return (out["path"], {k: v for k, v in out.items() if k != "path"}) if return_info else out["path"]

    def rollout_chain_samples(self, inner, dynamics, starts, n_steps, affine, n_samples=10, dt=1.0, nugget=None, random_state=0,
                              normals=None, x0=None, rtol=1e-10, max_passes=64, return_info=False):
        """rollout_samples() through a chain of transports: the paths of rollout_chain() when the dynamics is a function drawn from
        the posterior of `dynamics` (rollout_samples: arguments, conditioning, nugget — None: the noise level of `dynamics` —
        and normals).  Only the dynamics is sampled; the maps (this model the last, `inner` the ones before it, `affine` as
        pullback_chain's) act through their means: inverse, Jacobian and push-forward are rollout_chain's.  x0 (M,D): guesses
        of the source-space preimages of the starts.  Returns a dict: path (M,S,n_steps+1,D), steps_done, status (M,S) and,
        with return_info, vel, x, f, pvar, cvar (and chol for return_info="chol")."""
        maps = list(inner) + [self]
        affine = self._check_chain("rollout_chain_samples", maps, dynamics, affine, 1)
        return self._rollout_samples("rollout_chain_samples", maps, affine, dynamics, starts, n_steps, n_samples, dt, nugget, random_state,
                                     normals, x0, rtol, max_passes, return_info)

    def _rollout_samples(self, what, maps, affine, dynamics, starts, n_steps, n_samples, dt, nugget, random_state, normals, x0, rtol,
                         max_passes, return_info):
        starts, x0 = self._check_chain_points(what, starts, x0, rtol, max_passes, "starts")
        if int(n_steps) != n_steps or not 0 <= int(n_steps) <= _lib.ROLLOUT_SAMPLED_MAX_T:
            raise ValueError(f"{what}(): n_steps must be an integer 0 .. {_lib.ROLLOUT_SAMPLED_MAX_T} (_lib.ROLLOUT_SAMPLED_MAX_T), got {n_steps!r}")
        if int(n_samples) != n_samples or int(n_samples) < 1:
            raise ValueError(f"{what}(): n_samples must be an integer >= 1, got {n_samples!r}")
        if not np.isfinite(float(dt)) or float(dt) == 0.0:
            raise ValueError(f"{what}(): dt must be finite and not zero, got {dt!r}")
        nugget = float(dynamics._noise if nugget is None else nugget)
        if not np.isfinite(nugget) or nugget < 0.0:
            raise ValueError(f"{what}(): nugget must be finite and >= 0, got {nugget!r}")
        if len(dynamics.X) > _lib.ROLLOUT_STAB_MAX_N:
            raise ValueError(f"{what}(): the dynamics has {len(dynamics.X)} training points; the sampled rollout takes at most "
                             f"{_lib.ROLLOUT_STAB_MAX_N} (larger models: predict(return_cov=True) over the path so far, per step)")
        M, D = starts.shape
        S, T = int(n_samples), int(n_steps)
        if M * S * (T + 1) >= 2 ** 31:
            raise ValueError(f"{what}(): starts times n_samples times (n_steps + 1), the rows of the paths, must stay below 2^31")
        if normals is None:
            normals = np.random.RandomState(random_state).standard_normal((M, S, T, D))
        normals = _lib.as_f64(normals, 4, "normals")
        if normals.shape != (M, S, T, D):
            raise ValueError(f"{what}(): normals has shape {normals.shape}, expected (starts, n_samples, n_steps, D) = {(M, S, T, D)}")
        names = ("vel", "x", "f", "pvar", "cvar") + (("chol",) if return_info == "chol" else ()) if return_info else ()
        primary = lambda g: getattr(g._handle, "primary", g._handle)
        stages = [(primary(g), rot, src, dst, scale, jac) for g, (rot, scale, src, dst, jac) in zip(maps, affine)]
        out = primary(self).rollout_sampled(stages, primary(dynamics), np.repeat(starts, S, axis=0), normals.reshape(M * S, T, D), T, nugget,
                                            dt=float(dt), x0=None if x0 is None else np.repeat(x0, S, axis=0), rtol=rtol,
                                            max_passes=max_passes, outputs=names)
        return {k: v.reshape((M, S) + v.shape[1:]) for k, v in out.items()}       # path index = m * n_samples + j

    # ------------------------------------------------------------------ whole functions drawn from the posterior
    def sample_functions(self, n_functions=10, n_frequencies=2048, random_state=0, frequencies=None, draws=None):
        """n_functions whole functions drawn from the posterior of this model by pathwise conditioning (posterior_functions.py):
        the prior as a sum of n_frequencies random Fourier features, corrected by one solve against the training data per function
        on the device (_lib.Handle.apply_inverse).  Unlike the paths of rollout_samples(), each of which is a function of its own,
        these exist everywhere: they can be evaluated at any points (a sampled vector field), rolled out for any number of steps
        and from any number of starts under the same functions (PosteriorFunctions.predict / rollout), at a cost per step that
        does not grow with the step, for a model of any size.  The approximation is in the prior only: the covariance error falls
        as 1 / sqrt(n_frequencies); rollout_samples() stays the exact call for short paths.  The draws come from
        np.random.RandomState(random_state) in this order: the frequencies (posterior_functions.draw_frequencies), the amplitudes
        (draw_amplitudes), then eps = standard_normal((S, N, O)); V = apply_inverse(Y - prior_at(X) - sqrt(noise_var_) * eps), X and
        Y as fitted (NaN rows dropped).  frequencies (J,D): use these instead of drawing them.  draws = (w, eps): the standard
        normal numbers to use, w (S,J,2,O) for the amplitudes sqrt(c / J) * w and eps (S,N,O); zero draws give weights equal to
        alpha_, bit for bit, and functions equal to the posterior mean.  Needs n_outputs == n_features <= 3, float64, RBF or
        Matern 3/2 or 5/2 (the frequencies of Matern 1/2 do not converge usefully), at most _lib.PATHWISE_MAX_FREQ frequencies.
        Returns a PosteriorFunctions."""
        from .posterior_functions import sample_functions
        return sample_functions(self, n_functions, n_frequencies, random_state, frequencies, draws)

    def rollout_chain_functions(self, inner, functions, starts, n_steps, affine, dt=1.0, x0=None, rtol=1e-10, max_passes=64,
                                return_info=False):
        """PosteriorFunctions.rollout() through a chain of transports: the paths of rollout_chain() when the dynamics is, in turn,
        each of the `functions` drawn from its posterior (functions.gp is the dynamics; sample_functions()).  Only the dynamics is
        sampled; the maps (this model the last, `inner` the ones before it, `affine` as pullback_chain's) act through their
        means: inverse, Jacobian and push-forward are rollout_chain's.  Every start runs under every function.  x0 (M,D): guesses
        of the source-space preimages of the starts.  Returns a dict: path (M,S,n_steps+1,D), steps_done, status (M,S) and, with
        return_info, vel, x, f (M,S,n_steps,D)."""
        from .posterior_functions import PosteriorFunctions
        if not isinstance(functions, PosteriorFunctions):
            raise TypeError(f"rollout_chain_functions(): functions must be a PosteriorFunctions (GaussianProcess.sample_functions), got "
                            f"{type(functions).__name__}")
        maps = list(inner) + [self]
        affine = self._check_chain("rollout_chain_functions", maps, functions.gp, affine, 1)
        return functions._rollout("rollout_chain_functions", maps, affine, starts, n_steps, dt, x0, rtol, max_passes, return_info)

    # ------------------------------------------------------------------ fused metric path
    def prefetch_posterior(self, x):
        """Everything predict(x, return_std=True) and derivative(x, return_var=True) return, computed in ONE pass over
        the factor (the variance and the three Jacobian-variance columns share the 4-column kernel: 4 column passes
        instead of 1 + 4) and kept for the next calls with the same x.  Used by
        GaussianProcessTransportation.apply_transportation, which asks for both at the same positions."""
        self._require_fit()
        self._require_derivatives("prefetch_posterior")
        xk = np.array(x, dtype=np.float64, order="C", copy=True)
        self._memo = (xk, self._handle.predict_all(xk, mean=True, var=True, J=True, Jvar=True))

    def _memo_lookup(self, x):
        memo = getattr(self, "_memo", None)
        if memo is None:
            return None
        xk, out = memo
        x = np.asarray(x)
        if x.shape != xk.shape or not np.array_equal(x, xk):
            return None
        return out

    def posterior(self, x, jacobian_variance=False):
        """One call for mean (M,O), raw variance (M,), Jacobian (M,O,D) [and Jacobian variance (M,D)]."""
        self._require_fit()
        self._require_derivatives("posterior")
        return self._handle.predict_all(x, mean=True, var=True, J=True, Jvar=bool(jacobian_variance))
