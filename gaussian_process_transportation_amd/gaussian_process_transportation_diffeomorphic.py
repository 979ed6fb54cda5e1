"""GaussianProcessTransportationDiffeo — the reference's transport class that looks for a map without folds
(policy_transportation/transportation/gaussian_process_transportation_diffeomorphic.py:14-167), on this package's own classes.

The fitted map Phi = affine + psi is a diffeomorphism only where det(I + J_psi) > 0.  The reference searches the upper bound m of
the RBF length-scale with 100 optuna trials, each a six-start hyper-parameter fit of C(0.1) * RBF([2, ..], bounds [0.1, m]) +
WhiteKernel(1e-4) scored by how badly a second "inverse surrogate" GP (inputs: the targets, outputs: minus the displacements, same
kernel) undoes the map on the demonstration (:109-137).  Here

    * the trials are a deterministic grid, np.geomspace(2, 20, n_trials), not a sampler;
    * search="device": all trials are fitted by ONE device search (gpt_batch_optimize_bounded: every run with the bounds of its
      candidate) and scored by ONE scan (gpt_batch_fold_scan: per candidate the surrogate error, min det(I + J_psi) and the count
      of det <= 0 on the evaluation set);  search="host": the same trials as a loop over GaussianProcess fits scored in numpy
      with predict / derivative, for any N;
    * criterion="error" is the reference's; criterion="fold_free" (default) picks, among the candidates that do not fold on the
      evaluation set, the one of highest log-marginal likelihood.  On the letter-S demo the reference's criterion picks m = 2,
      which folds at 10 of 400 points; the fold-free window is m in [3.3, 4.4] (README);
    * the map is then fitted AT the winning trial's theta (optimizer=None), so the map in use is the one that was scored;
      reference_refit=True reproduces the reference's second optimisation with bounds [1, m] instead (:149-150);
    * check_invertibility() does not overwrite training_traj (the reference does, :114, so a later apply_transportation()
      transports twice there).

Everything else — fit_transportation, apply_transportation, sample_transportation, inverse_transport, transported_policy,
rollout_policy, fused=True — is GaussianProcessTransportation's code; unlike that class, and as the reference's Diffeo class,
fit_transportation() reads `kernel_transport` when it is called and leaves the fitted kernel there (:59-63)."""
import warnings

import numpy as np

from . import _lib
from .gaussian_process import GaussianProcess
from .gaussian_process_transportation import GaussianProcessTransportation, _reference_default_kernel
from .policy_transportation import PolicyTransportation

DEVICE_MAX_N, DEVICE_MAX_D = _lib.BATCH_MAX_N, _lib.FOLD_SCAN_MAX_D
CRITERIA = ("fold_free", "error")
TRIAL_ALPHA = 1e-10                                       # GaussianProcess's default jitter, the reference's


def trial_kernel(max_lengthscale, D):
    """C(0.1) * RBF(2 ones(D), length_scale_bounds=[0.1, m]) + WhiteKernel(1e-4): the reference's trial kernel (:125)."""
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    return ConstantKernel(0.1) * RBF(length_scale=2.0 * np.ones(D), length_scale_bounds=[0.1, float(max_lengthscale)]) + WhiteKernel(0.0001)


def select_trial(criterion, lml, error, min_det, n_fold, status, surrogate_status=None):
    """(index, fell_back): the candidate optimize_diffeomorphism picks from per-candidate arrays.
    "error": the lowest surrogate error among the candidates that have one (status and surrogate_status GPT_OK, error not NaN), the
    first on ties.  "fold_free": among the candidates with status GPT_OK, n_fold == 0 and a finite LML the highest LML, the first
    on ties; if there is none, the largest min_det among those with status GPT_OK, and fell_back is True."""
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}, got {criterion!r}")
    lml, error, min_det = (np.asarray(a, dtype=np.float64) for a in (lml, error, min_det))
    n_fold, ok = np.asarray(n_fold), np.asarray(status) == _lib.GPT_OK
    if not ok.any():
        raise np.linalg.LinAlgError("optimize_diffeomorphism: no candidate has a positive definite matrix")
    if criterion == "error":
        has = ok & ~np.isnan(error)
        if surrogate_status is not None:
            has &= np.asarray(surrogate_status) == _lib.GPT_OK
        if not has.any():
            raise np.linalg.LinAlgError("optimize_diffeomorphism: no candidate has a surrogate error (its matrix is not positive definite)")
        return int(np.flatnonzero(has)[np.argmin(error[has])]), False
    free = ok & (n_fold == 0) & np.isfinite(lml)
    if free.any():
        return int(np.flatnonzero(free)[np.argmax(lml[free])]), False
    return int(np.flatnonzero(ok)[np.argmax(min_det[ok])]), True


def _det_i_plus(J):
    return np.linalg.det(J + np.eye(J.shape[-1]))


class GaussianProcessTransportationDiffeo(GaussianProcessTransportation):
    def __init__(self, kernel_transport=None, optimizer="fmin_l_bfgs_b", device=0, verbose=True, devices=None, matern_derivatives=False,
                 fused=False):
        """Arguments as GaussianProcessTransportation's; kernel_transport defaults to the reference's (:15)."""
        self.kernel_transport = _reference_default_kernel() if kernel_transport is None else kernel_transport
        self.optimizer, self.device, self.verbose, self.devices = optimizer, device, verbose, devices
        self.matern_derivatives = matern_derivatives
        super().__init__(self.kernel_transport, optimizer=optimizer, device=device, verbose=verbose, devices=devices,
                         matern_derivatives=matern_derivatives, fused=fused)

    # ------------------------------------------------------------------ the reference's protocol
    def _regressor(self, kernel, optimize):
        return GaussianProcess(kernel=kernel, optimizer=self.optimizer if optimize else None, n_restarts_optimizer=5, device=self.device,
                               verbose=self.verbose, devices=self.devices, matern_derivatives=self.matern_derivatives)

    def fit_transportation(self, optimize=True, do_scale=False, do_rotation=True):
        """Affine pre-alignment + GP fit of the residual displacement field from `kernel_transport` as it stands now, with 5
        restarts (optimize=True) or at the kernel's own hyper-parameters (:48-63)."""
        if self.verbose:
            print("Kernel:", self.kernel_transport)
        self.method = PolicyTransportation(self._regressor(self.kernel_transport, optimize), verbose=self.verbose)
        super().fit_transportation(do_scale=do_scale, do_rotation=do_rotation)
        self.affine_transform = self.method.affine_transform
        self.delta_distribution = self.method.delta_distribution
        self.gp_delta_map = self.method.delta_map
        self.kernel_transport = self.gp_delta_map.kernel

    def apply_transportation(self):
        """GaussianProcessTransportation.apply_transportation(), then the reference's extra attributes traj_rotated and
        delta_map_mean (:70-72)."""
        before = self._input("training_traj")
        super().apply_transportation()
        self.traj_rotated = self.affine_transform.predict(before)
        self.delta_map_mean = self.gp_delta_map.predict(self.traj_rotated)

    # ------------------------------------------------------------------ scoring
    def _fitted(self):
        gp = getattr(self, "gp_delta_map", None)
        if gp is None or gp._handle is None:
            raise RuntimeError("GaussianProcessTransportationDiffeo: call fit_transportation() first")
        return gp

    @staticmethod
    def _device_refusal(n, D, what):
        if n > DEVICE_MAX_N or D > DEVICE_MAX_D:
            return (f"{what}: the device path needs n <= {DEVICE_MAX_N} source points and D <= {DEVICE_MAX_D}, got n = {n}, D = {D}; "
                    'use search="host"')
        return None

    def _scan_device(self, X, Y, hyper, points, surrogate=True, per_query=False):
        """One gpt_batch_fold_scan call for B candidates (c, ls, noise) over the data set (X, Y) at `points`."""
        B = len(hyper)
        n_begin = np.arange(B + 1, dtype=np.int64) * X.shape[0]
        return _lib.batch_fold_scan_packed(np.tile(X, (B, 1)), np.tile(Y, (B, 1)), n_begin, np.array([h[1] for h in hyper]),
                                           np.array([h[0] for h in hyper]), np.array([h[2] for h in hyper]), TRIAL_ALPHA, points, None,
                                           surrogate, per_query, 0, self.device)

    def _score_host(self, gp, points):
        """The scan's numbers for one fitted GaussianProcess from its predict / derivative calls, in numpy."""
        psi = gp.predict(points).reshape(len(points), -1)
        det = _det_i_plus(gp.derivative(points))
        z = points + psi
        out = dict(status=_lib.GPT_OK, min_det=float(det.min()), argmin=int(np.argmin(det)), n_fold=int((det <= 0).sum()), det=det, z=z,
                   psi=psi, surrogate_status=_lib.GPT_OK, error=np.nan, err_max=np.nan)
        inv = GaussianProcess(kernel=gp.kernel, alpha=gp.alpha, optimizer=None, device=self.device, verbose=False)
        try:
            inv.fit(gp.X + gp.Y, -gp.Y)                    # the targets, minus the displacements (:115-117)
        except np.linalg.LinAlgError:
            out["surrogate_status"] = _lib.GPT_E_NOT_PD
            return out
        psi_inv = inv.predict(z).reshape(len(points), -1)
        err = np.linalg.norm(psi + psi_inv, axis=1)
        out.update(error=float(err.sum()), err_max=float(err.max()), psi_inv=psi_inv)
        return out

    def check_invertibility(self):
        """The reference's number (:109-121): sum over the demonstration of |delta + delta_inv|, delta the map's displacement at
        the affine-moved trajectory and delta_inv the inverse surrogate's at the moved points.  Also sets delta_map_mean,
        delta_map_inv_mean, traj_rotated, traj_rotated_inv, min_det_ and n_fold_ (det(I + J_psi) over the trajectory).
        training_traj is left as it is."""
        gp = self._fitted()
        self.traj_rotated = self.affine_transform.predict(self._input("training_traj"))
        n, D = gp.X.shape
        if gp._ktype != 0 or self._device_refusal(n, D, "") or gp.Y.shape[1] != D:
            s = self._score_host(gp, self.traj_rotated)
            if s["surrogate_status"] != _lib.GPT_OK:
                raise np.linalg.LinAlgError("check_invertibility: the inverse surrogate's matrix is not positive definite")
            z, psi_inv, error = s["z"], s["psi_inv"], s["error"]
            self.min_det_, self.n_fold_ = s["min_det"], s["n_fold"]
        else:
            s = self._scan_device(gp.X, gp.Y, [(gp._c, gp._ls, gp._noise)], self.traj_rotated, per_query=True)
            if s["status"][0] != _lib.GPT_OK or s["surrogate_status"][0] != _lib.GPT_OK:
                raise np.linalg.LinAlgError("check_invertibility: the map's or the inverse surrogate's matrix is not positive definite")
            z, error = s["z"][0], float(s["err_sum"][0])
            self.min_det_, self.n_fold_ = float(s["min_det"][0]), int(s["n_fold"][0])
            out, _ = _lib.batch_predict([gp.X + gp.Y], [-gp.Y], gp._ls[None, :], [gp._c], [gp._noise], gp.alpha, [z], device=self.device, mean=True)
            psi_inv = out["mean"][0]
        self.delta_map_mean = z - self.traj_rotated
        self.delta_map_inv_mean = psi_inv
        self.traj_rotated_inv = z + psi_inv
        return error

    # ------------------------------------------------------------------ the search
    def _prepare(self, do_scale, do_rotation):
        from .affine_transform import AffineTransform
        source, target = self._input("source_distribution"), self._input("target_distribution")
        aff = AffineTransform(do_scale=do_scale, do_rotation=do_rotation, verbose=False).fit(source, target)
        X = aff.predict(source)
        return aff, X, np.asarray(target, dtype=np.float64) - X

    def _run_trials(self, ms, search, points, X, Y):
        """diffeo_trials_ for the candidates ms."""
        D, B = X.shape[1], len(ms)
        kernels = [trial_kernel(m, D) for m in ms]
        t = dict(max_lengthscale=np.array(ms, dtype=np.float64), theta=np.full((B, 2 + D), np.nan), lml=np.full(B, np.nan),
                 error=np.full(B, np.nan), min_det=np.full(B, np.nan), argmin=np.full(B, -1, dtype=np.int64),
                 n_fold=np.full(B, -1, dtype=np.int64), status=np.zeros(B, dtype=np.int32), surrogate_status=np.zeros(B, dtype=np.int32))
        if search == "device":
            msg = self._device_refusal(X.shape[0], D, "optimize_diffeomorphism(search=\"device\")")
            if msg:
                raise ValueError(msg)
            from .batch_hyperopt import optimize_hyperparameters_candidates
            stats = {}
            fits = optimize_hyperparameters_candidates(kernels, X, Y, alpha=TRIAL_ALPHA, n_restarts_optimizer=5, device=self.device, stats=stats)
            s = self._scan_device(X, Y, fits, points)
            t.update(lml=np.array([f[3] for f in fits]), theta=np.array([f[4] for f in fits]), error=s["err_sum"], min_det=s["min_det"],
                     argmin=s["argmin"], n_fold=s["n_fold"], status=s["status"], surrogate_status=s["surrogate_status"])
            self.diffeo_search_stats_ = stats
            return t
        if search != "host":
            raise ValueError(f'search must be "device" or "host", got {search!r}')
        for k, kernel in enumerate(kernels):
            gp = GaussianProcess(kernel=kernel, alpha=TRIAL_ALPHA, n_restarts_optimizer=5, device=self.device, verbose=False)
            try:
                gp.fit(X, Y)
            except np.linalg.LinAlgError:
                t["status"][k] = _lib.GPT_E_NOT_PD
                continue
            s = self._score_host(gp, points)
            t["theta"][k], t["lml"][k] = gp.kernel.theta, gp.gp.log_marginal_likelihood_value_
            t["error"][k], t["min_det"][k], t["argmin"][k], t["n_fold"][k] = s["error"], s["min_det"], s["argmin"], s["n_fold"]
            t["surrogate_status"][k] = s["surrogate_status"]
        return t

    def diffeomorphism_error(self, max_lengthscale, search="device", do_scale=False, do_rotation=True):
        """One trial (:123-137): the map fitted with the length-scale ceiling `max_lengthscale` — a float, or any object with
        suggest_float (an optuna trial: the ceiling is trial.suggest_float("max_lengthscale", 2, 20, log=True)) — and the surrogate
        error of that fit on the affine-moved trajectory.  Leaves the fitted map in place, as the reference does."""
        if hasattr(max_lengthscale, "suggest_float"):
            max_lengthscale = max_lengthscale.suggest_float("max_lengthscale", 2, 20, log=True)
        aff, X, Y = self._prepare(do_scale, do_rotation)
        t = self._run_trials([float(max_lengthscale)], search, aff.predict(self._input("training_traj")), X, Y)
        if t["status"][0] != _lib.GPT_OK or t["surrogate_status"][0] != _lib.GPT_OK:
            raise np.linalg.LinAlgError("diffeomorphism_error: the map's or the inverse surrogate's matrix is not positive definite")
        self._fit_at(trial_kernel(max_lengthscale, X.shape[1]).clone_with_theta(t["theta"][0]), do_scale, do_rotation)
        return float(t["error"][0])

    def _fit_at(self, kernel, do_scale, do_rotation):
        verbose, self.verbose = self.verbose, False
        try:
            self.kernel_transport = kernel
            self.fit_transportation(optimize=False, do_scale=do_scale, do_rotation=do_rotation)
        finally:
            self.verbose = verbose

    def optimize_diffeomorphism(self, n_trials=100, max_lengthscales=None, criterion="fold_free", eval_points=None, search="device",
                                reference_refit=False, do_scale=False, do_rotation=True):
        """Searches the length-scale ceiling (:139-150) and fits the map at the winner.  max_lengthscales: the candidates (default
        np.geomspace(2, 20, n_trials)).  eval_points (M, D): where the map is scored, in the space psi acts on, i.e. after the
        affine part (default: the affine-moved training_traj, as the reference; e.g. the grid a rollout will cover).
        Sets diffeo_trials_ (per-candidate arrays max_lengthscale, theta, lml, error, min_det, argmin, n_fold, status,
        surrogate_status), max_lengthscale_, and fold_free_: whether the map now in place has det(I + J_psi) > 0 on the whole
        evaluation set.  search="device" needs n <= 128 source points and D <= 3; search="host" works for any N."""
        if criterion not in CRITERIA:
            raise ValueError(f"criterion must be one of {CRITERIA}, got {criterion!r}")
        ms = np.geomspace(2, 20, int(n_trials)) if max_lengthscales is None else np.atleast_1d(np.asarray(max_lengthscales, dtype=np.float64))
        if ms.size < 1 or not (np.isfinite(ms).all() and (ms > 0.1).all()):
            raise ValueError("optimize_diffeomorphism: the candidates must be finite and above the lower length-scale bound 0.1")
        aff, X, Y = self._prepare(do_scale, do_rotation)
        points = aff.predict(self._input("training_traj")) if eval_points is None else _lib.as_f64(eval_points, 2, "eval_points")
        if points.shape[1] != X.shape[1]:
            raise ValueError(f"optimize_diffeomorphism: eval_points must have {X.shape[1]} columns")
        t = self._run_trials(list(ms), search, points, X, Y)
        best, fell_back = select_trial(criterion, t["lml"], t["error"], t["min_det"], t["n_fold"], t["status"], t["surrogate_status"])
        if fell_back:
            warnings.warn(f"optimize_diffeomorphism: every candidate folds on the evaluation set; keeping the one with the largest "
                          f"min det(I + J_psi) = {t['min_det'][best]:.3g} (max_lengthscale = {ms[best]:.4g}, folds at {int(t['n_fold'][best])} points)")
        self.diffeo_trials_, self.max_lengthscale_ = t, float(ms[best])
        D = X.shape[1]
        if reference_refit:                                # the reference's second optimisation (:149-150)
            from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
            self.kernel_transport = ConstantKernel(0.1) * RBF(length_scale=np.ones(D), length_scale_bounds=[1, float(ms[best])]) + WhiteKernel(0.0001)
            verbose, self.verbose = self.verbose, False
            try:
                self.fit_transportation(optimize=True, do_scale=do_scale, do_rotation=do_rotation)
            finally:
                self.verbose = verbose
        else:
            self._fit_at(trial_kernel(ms[best], D).clone_with_theta(t["theta"][best]), do_scale, do_rotation)
        gp = self.gp_delta_map
        if search == "device":
            s = self._scan_device(gp.X, gp.Y, [(gp._c, gp._ls, gp._noise)], points, surrogate=False)
            self.fold_free_ = bool(s["status"][0] == _lib.GPT_OK and s["n_fold"][0] == 0)
        else:
            self.fold_free_ = bool((_det_i_plus(gp.derivative(points)) > 0).all())
        if self.verbose:
            print(f"optimize_diffeomorphism: {ms.size} trials, criterion {criterion}: max_lengthscale = {ms[best]:.4g}, "
                  f"fold-free on the evaluation set: {self.fold_free_}")
        return self.max_lengthscale_
