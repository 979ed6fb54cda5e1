"""GaussianProcessTransportationBatch — the attribute protocol of GaussianProcessTransportation
(policy_transportation/transportation/gaussian_process_transportation.py:11-30) for many independent (source, target)
pairs at once, the per-frame loop of the reference's multi-frame model
(example/comparisons/multi_reference_frames/models/model_gpt.py:74-83) as one batch.

Protocol (list-valued; entry b belongs to pair b):
    inputs   source_distributions, target_distributions [(n_b, D)], training_trajs [(M_b, D)], optional training_deltas [(M_b, D)]
    calls    fit_transportations(do_scale=False, do_rotation=True), apply_transportations()
    outputs  training_trajs (moved), stds, training_trajs_old, and with velocities training_deltas + var_vels_transported

Each pair's AffineTransform runs on the host.  The displacement GPs of all pairs are fitted by one GaussianProcessBatch.fit
and evaluated by one batched posterior call; the push-forward algebra is PolicyTransportation's own, run per pair on an
adapter that serves that pair's share of the batch's results.  Orientations and sampling stay with the single-model class."""
import numpy as np

from .gaussian_process_batch import GaussianProcessBatch
from .gaussian_process_transportation import _MISSING, _reference_default_kernel
from .policy_transportation import PolicyTransportation


class _Member:
    """The delta_map PolicyTransportation sees for one pair: records what it is asked to fit, and answers predict /
    derivative at the positions the batch was evaluated at."""

    def __init__(self, batch, index):
        self.batch, self.index = batch, index
        self.fit_X = self.fit_Y = None
        self.served = None                      # (positions, posterior dict)

    def fit(self, X, Y):
        self.fit_X, self.fit_Y = X, Y

    def _at(self, x):
        if self.served is None or np.shape(x) != self.served[0].shape or not np.array_equal(x, self.served[0]):
            raise RuntimeError("GaussianProcessTransportationBatch: a pair asked for positions the batch was not evaluated at")
        return self.served[1]

    def predict(self, x, return_std=False):
        out = self._at(x)
        return self.batch._member_predict(self.index, out["mean"], out["var"] if return_std else None)

    def derivative(self, x, return_var=False):
        out = self._at(x)
        return self.batch._member_derivative(self.index, out["J"], out["Jvar"] if return_var else None)


class GaussianProcessTransportationBatch:
    def __init__(self, kernel_transport=None, optimizer="fmin_l_bfgs_b", n_restarts_optimizer=5, device=0, verbose=False):
        kernel = _reference_default_kernel() if kernel_transport is None else kernel_transport
        self.regressor = GaussianProcessBatch(kernel=kernel, optimizer=optimizer, n_restarts_optimizer=n_restarts_optimizer,
                                              device=device, verbose=verbose)
        self.verbose = verbose
        self.methods = []

    def _input(self, name):
        value = getattr(self, name, _MISSING)
        if value is _MISSING:
            raise AttributeError(f"GaussianProcessTransportationBatch: set .{name} before this call")
        return list(value)

    def fit_transportations(self, do_scale=False, do_rotation=True):
        """Per pair the affine pre-alignment (host), then one batched fit of the residual displacement fields."""
        sources, targets = self._input("source_distributions"), self._input("target_distributions")
        if len(sources) != len(targets):
            raise ValueError(f"GaussianProcessTransportationBatch: {len(sources)} sources but {len(targets)} targets")
        self.methods = [PolicyTransportation(_Member(self.regressor, b), verbose=self.verbose) for b in range(len(sources))]
        for method, source, target in zip(self.methods, sources, targets):
            method.fit(source, target, do_scale=do_scale, do_rotation=do_rotation)
        self.regressor.fit([m.delta_map.fit_X for m in self.methods], [m.delta_map.fit_Y for m in self.methods])

    def apply_transportations(self):
        """Moves every demonstration; velocities follow when they were provided."""
        if not self.methods:
            raise RuntimeError("GaussianProcessTransportationBatch: fit_transportations() first")
        before = self._input("training_trajs")
        if len(before) != len(self.methods):
            raise ValueError(f"GaussianProcessTransportationBatch: {len(before)} trajectories for {len(self.methods)} pairs")
        velocities = getattr(self, "training_deltas", _MISSING)
        with_vel = velocities is not _MISSING
        rotated = [np.array(m.affine_transform.predict(x), dtype=np.float64, order="C") for m, x in zip(self.methods, before)]
        if with_vel:
            posterior = self.regressor.posterior(rotated, jacobian_variance=True)
        else:
            out = self.regressor._posterior(rotated, "apply_transportations", mean=True, var=True)
            posterior = [{k: v[b] for k, v in out.items()} for b in range(len(rotated))]
        self.training_trajs_old = before
        moved, stds, vels, var_vels = [], [], [], []
        for b, method in enumerate(self.methods):
            method.delta_map.served = (rotated[b], posterior[b])
            traj, std = method.transport(before[b])
            moved.append(traj)
            stds.append(std)
            if with_vel:
                vel, var_vel = method.transport_velocity(before[b], list(velocities)[b])
                vels.append(vel)
                var_vels.append(var_vel)
        self.training_trajs, self.stds = moved, stds
        if with_vel:
            self.training_deltas, self.var_vels_transported = vels, var_vels
