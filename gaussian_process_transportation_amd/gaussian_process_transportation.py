"""GaussianProcessTransportation — the user-facing attribute protocol of the reference
(policy_transportation/transportation/gaussian_process_transportation.py:11-30).

Protocol (names are the reference's, they are the API):
    inputs   source_distribution (N,D), target_distribution (N,D), training_traj (M,D)
             optional training_delta (M,D) velocities, training_ori (M,4) quaternions (D = 3)
    calls    fit_transportation(do_scale=False, do_rotation=True), apply_transportation(), sample_transportation()
    outputs  training_traj (moved), std, training_traj_old, and for the optional inputs
             training_delta + var_vel_transported, training_ori

The regressor behind it is the MI355X GaussianProcess; as in the reference the kernel is consumed by the
constructor, so assigning `.kernel_transport` afterwards changes nothing."""
from .gaussian_process import GaussianProcess
from .policy_transportation import PolicyTransportation

_MISSING = object()


def _reference_default_kernel():
    """C(0.1) * RBF([0.1]) + WhiteKernel(1e-4): the default argument of the reference's constructor (:12)."""
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    return ConstantKernel(0.1) * RBF(length_scale=[0.1]) + WhiteKernel(0.0001)


class GaussianProcessTransportation:
    def __init__(self, kernel_transport=None, optimizer="fmin_l_bfgs_b", device=0, verbose=True, devices=None,
                 matern_derivatives=False, fused=False):
        """`devices=[0, 1, ...]`: apply_transportation() shards the demonstration's rows over these GPUs (the fit stays on
        devices[0]); default: the one `device`.  `matern_derivatives=True`: a Matern(nu=1.5 / 2.5) kernel_transport
        transports velocities and orientations with the analytic derivatives of its posterior (GaussianProcess).
        `fused=True`: apply_transportation() is one call (PolicyTransportation.transport_all: the affine part, the posterior
        and the velocity / orientation algebra on the device, on the GPU that holds the fit) and sets the same attributes."""
        self.fused = bool(fused)
        kernel = _reference_default_kernel() if kernel_transport is None else kernel_transport
        regressor = GaussianProcess(kernel=kernel, optimizer=optimizer, device=device, verbose=verbose, devices=devices,
                                    matern_derivatives=matern_derivatives)
        self.method = PolicyTransportation(regressor, verbose=verbose)

    def _input(self, name):
        value = getattr(self, name, _MISSING)
        if value is _MISSING:
            raise AttributeError(f"GaussianProcessTransportation: set .{name} before this call")
        return value

    def fit_transportation(self, do_scale=False, do_rotation=True):
        """Affine pre-alignment + GP fit of the residual displacement field (policy_transportation.py:16-24)."""
        source, target = self._input("source_distribution"), self._input("target_distribution")
        self.method.fit(source, target, do_scale=do_scale, do_rotation=do_rotation)

    def apply_transportation(self):
        """Moves the demonstration; velocities and orientations follow when they were provided (:19-27).  fused=True treats
        training_delta / training_ori set to None as not provided; the unfused path, as the reference, skips only an
        attribute that was never set and hands a None on to numpy, which fails."""
        before = self._input("training_traj")
        self.training_traj_old = before
        if self.fused:
            velocities, orientations = getattr(self, "training_delta", None), getattr(self, "training_ori", None)
            traj, std, vel, var_vel, ori = self.method.transport_all(before, velocities, orientations)
            self.training_traj, self.std = traj, std
            if velocities is not None:
                self.training_delta, self.var_vel_transported = vel, var_vel
            if orientations is not None:
                self.training_ori = ori
            return
        velocities = getattr(self, "training_delta", _MISSING)
        if velocities is not _MISSING:
            self.method.prefetch(before)              # std and Jacobian variance at the same positions: one pass
        self.training_traj, self.std = self.method.transport(before)
        if velocities is not _MISSING:
            self.training_delta, self.var_vel_transported = self.method.transport_velocity(before, velocities)
        orientations = getattr(self, "training_ori", _MISSING)
        if orientations is not _MISSING:
            self.training_ori = self.method.transport_orientation(before, orientations)

    def inverse_transport(self, points, x0=None, return_info=False, **solver):
        """The points that fit_transportation()'s map sends to `points` (an addition: PolicyTransportation.inverse_transport);
        x0: a guess of them, return_info: also status / passes / residual / det per point, solver: rtol, max_passes."""
        return self.method.inverse_transport(points, x0=x0, return_info=return_info, **solver)

    def transported_policy(self, dynamics, points, x0=None, return_std=False, return_info=False, **solver):
        """The transported policy at `points` of the target scene (an addition: PolicyTransportation.transported_policy):
        the velocities a `dynamics` GaussianProcess fitted on the source demonstration commands there, pulled back through
        fit_transportation()'s map; x0: a guess of the preimages, return_std: also their std, return_info: also x / status /
        passes / residual / det / f per point, solver: rtol, max_passes."""
        return self.method.transported_policy(dynamics, points, x0=x0, return_std=return_std, return_info=return_info, **solver)

    def rollout_policy(self, dynamics, starts, n_steps, dt=1.0, x0=None, return_info=False, variance_gain=None, **solver):
        """The paths the transported policy drives from `starts` of the target scene, n_steps steps of size dt, integrated on
        the device in one call (an addition: PolicyTransportation.rollout_policy)."""
        return self.method.rollout_policy(dynamics, starts, n_steps, dt=dt, x0=x0, return_info=return_info, variance_gain=variance_gain,
                                          **solver)

    def rollout_policy_samples(self, dynamics, starts, n_steps, n_samples=10, dt=1.0, nugget=None, random_state=0, normals=None,
                               x0=None, return_info=False, **solver):
        """n_samples paths per start of rollout_policy() when the dynamics is a function drawn from the posterior of `dynamics`,
        each draw conditioned on the path's own earlier ones, in one device call (an addition:
        PolicyTransportation.rollout_policy_samples).  Only the dynamics is sampled; the map acts through its mean."""
        return self.method.rollout_policy_samples(dynamics, starts, n_steps, n_samples=n_samples, dt=dt, nugget=nugget,
                                                  random_state=random_state, normals=normals, x0=x0, return_info=return_info, **solver)

    def rollout_policy_functions(self, functions, starts, n_steps, dt=1.0, x0=None, return_info=False, **solver):
        """The paths of rollout_policy() from every start under each of `functions`, whole functions drawn from the posterior of the
        dynamics (GaussianProcess.sample_functions), any number of steps, in one device call (an addition:
        PolicyTransportation.rollout_policy_functions).  Only the dynamics is sampled; the map acts through its mean."""
        return self.method.rollout_policy_functions(functions, starts, n_steps, dt=dt, x0=x0, return_info=return_info, **solver)

    def sample_transportation(self):
        """Posterior draws of the moved demonstration, at the positions of the last apply_transportation() (:29-30)."""
        return self.method.sample_transportation(self._input("training_traj_old"))
