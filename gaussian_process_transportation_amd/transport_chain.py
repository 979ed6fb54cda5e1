"""TransportChain — several fitted transports applied one after the other, Phi = Phi_{K-1} o ... o Phi_0, as the reference's
obstacle example does by hand (example/2D/surface_generalization_with_obstacle.py:142-200: a first transport from the old surface
to the new one, a second, fitted in the new scene, round an obstacle).  The reference then refits a GP on the twice-moved
demonstration to get a velocity field; here the source dynamics is pulled back through all the maps in ONE device call
(GaussianProcess.pullback_chain): K inverses, the dynamics mean and the push-forward, with the variance of every map and of the
dynamics carried through the maps after it."""
import numpy as np

from . import _lib


class TransportChain:
    def __init__(self, transports, verbose=True):
        """`transports`: 1 .. 4 fitted GaussianProcessTransportation (or PolicyTransportation) objects in the order they are
        applied, all of one dimension, each with a delta_map that has `pullback_policy` (GaussianProcess)."""
        transports = list(transports)
        if not 1 <= len(transports) <= _lib.CHAIN_MAX:
            raise ValueError(f"TransportChain: 1 .. {_lib.CHAIN_MAX} transports, got {len(transports)}")
        self.methods = [getattr(t, "method", t) for t in transports]          # the PolicyTransportation behind each
        dims = []
        for k, m in enumerate(self.methods):
            if getattr(m, "affine_transform", None) is None or not hasattr(m.affine_transform, "rotation_matrix"):
                raise RuntimeError(f"TransportChain: transport {k} is not fitted (fit_transportation() comes first)")
            if getattr(m.delta_map, "pullback_policy", None) is None or getattr(m.delta_map, "pullback_chain", None) is None:
                raise NotImplementedError(f"TransportChain: the delta_map of transport {k} ({type(m.delta_map).__name__}) has no "
                                          "pullback_policy / pullback_chain; GaussianProcess provides them")
            dims.append(int(np.shape(m.affine_transform.rotation_matrix)[0]))
        if len(set(dims)) != 1:
            raise ValueError(f"TransportChain: the transports must share one space, got dimensions {dims}")
        self.n_features = dims[0]
        self.verbose = verbose

    def __len__(self):
        return len(self.methods)

    def transport(self, points, vel=None, ori=None):
        """The forward composition: every stage's transport_all in turn, the positions, velocities and orientations of one
        stage the inputs of the next (a host loop over the existing calls).  Returns (positions, velocities, orientations,
        [std of stage 0, std of stage 1, ...]); None for what was not given."""
        pos, stds = np.asarray(points, dtype=np.float64), []
        for m in self.methods:
            verbose, m.verbose = m.verbose, m.verbose and self.verbose
            try:
                pos, std, vel, _, ori = m.transport_all(pos, vel, ori)
            finally:
                m.verbose = verbose
            stds.append(std)
        return pos, vel, ori, stds

    def _pull(self, dynamics, points, x0, variances, solver, outputs=None):
        unknown = set(solver) - {"rtol", "max_passes"}
        if unknown:
            raise TypeError(f"TransportChain: unknown solver arguments {sorted(unknown)}")
        affine = [(m.affine_transform.rotation_matrix, m.affine_transform.scale, m.affine_transform.S_centroid,
                   m.affine_transform.T_centroid, m.affine_transform.rotation_matrix) for m in self.methods]
        maps = [m.delta_map for m in self.methods]
        if outputs is not None and self.verbose:
            outputs = tuple(outputs) + ("stage_status", "stage_det")
        out = maps[-1].pullback_chain(maps[:-1], dynamics, np.asarray(points, dtype=np.float64), affine, x0=x0, variances=variances,
                                      outputs=outputs, **solver)
        if self.verbose:
            for k in range(len(maps) - 1, -1, -1):
                status = out["stage_status"][k]
                counts = ", ".join(f"{name} {int(np.sum(status == code))}" for code, name in enumerate(_lib.INV_STATUS_NAMES))
                solved = status == _lib.INV_CONVERGED
                print(f"Inverse of map {k}: {counts}; det(I + J_psi) <= 0 at {int(np.sum(out['stage_det'][k][solved] <= 0))} "
                      f"of {int(np.sum(solved))} solutions")
        return out

    def transported_policy(self, dynamics, points, x0=None, return_std=False, return_info=False, **solver):
        """The transported policy at `points` (M,D) of the LAST scene: the velocity J_Phi(x) dynamics.predict(x) at
        x = Phi^-1(points), `dynamics` a GaussianProcess fitted on the source demonstration.  x0: a guess of the source-space
        preimages; `solver` passes rtol / max_passes on.  Returns the velocities (M,D); with return_std also std (M,D) =
        sqrt(vel_var_dyn + vel_var_map); with return_info also a dict: x, f, status (the first stage in solve order that did
        not converge) and the per-stage arrays stage_x, stage_z, stage_A, stage_status, stage_passes, stage_residual,
        stage_det (K,M,...), with return_std also var_dyn, vel_var_dyn, vel_var_map, stage_Jvar, stage_map_var.  Velocities
        use the reference's unscaled Jacobian of each affine part (AffineTransform.derivative)."""
        # without the dict only what is returned leaves the device: at a handful of points the copies are most of the call
        lean = None if return_info else ("vel_var_dyn", "vel_var_map") if return_std else ()
        out = self._pull(dynamics, points, x0, (True if return_info else "vel") if return_std else False, solver, outputs=lean)
        res = (out["vel"],)
        if return_std:
            res += (np.sqrt(out["vel_var_dyn"] + out["vel_var_map"]),)
        if return_info:
            res += ({k: v for k, v in out.items() if k != "vel"},)
        return res if len(res) > 1 else res[0]

    def rollout(self, dynamics, starts, n_steps, dt=1.0, x0=None, return_info=False, variance_gain=None, **solver):
        """The paths the transported policy drives from `starts` (M,D) of the LAST scene: n_steps explicit Euler steps
        y_{t+1} = y_t + dt * transported_policy(dynamics, y_t), the x of one step the guess of the next (x0: guesses for the
        starts), the loop over the steps on the device in ONE call (GaussianProcess.rollout_chain) — equal, bit for bit, to the
        host loop over transported_policy(dynamics, y_t, x0=x_{t-1}) that the reference's plot_traj_evolution runs.  dt: finite,
        not zero; negative integrates backwards.  `solver` passes rtol / max_passes on.  Returns path (M,n_steps+1,D), row 0 the
        starts; a trajectory ends at the first step whose inverse does not converge or whose next point is not finite, and its
        rows after that are NaN.  With return_info also a dict: vel, x (M,n_steps,D), steps_done (M,) and status (M,), the
        _lib.INV_* of the last step evaluated.  variance_gain=None: the mean policy only, as described.  A number >= 0: the
        variance-stabilised step (GaussianProcess.rollout_chain), vel_t = push(f_t - variance_gain * std_t * grad_var_t /
        |grad_var_t|) with the dynamics' own standard deviation and variance gradient at the preimage x_t, still one device call;
        the info dict then also holds f, var (M,n_steps) and dvar."""
        unknown = set(solver) - {"rtol", "max_passes"}
        if unknown:
            raise TypeError(f"TransportChain: unknown solver arguments {sorted(unknown)}")
        rollout = getattr(self.methods[-1].delta_map, "rollout_chain", None)
        if rollout is None:
            raise NotImplementedError(f"TransportChain.rollout(): the delta_map of the last transport ({type(self.methods[-1].delta_map).__name__}) "
                                      "has no rollout_chain; GaussianProcess provides one")
        affine = [(m.affine_transform.rotation_matrix, m.affine_transform.scale, m.affine_transform.S_centroid,
                   m.affine_transform.T_centroid, m.affine_transform.rotation_matrix) for m in self.methods]
        maps = [m.delta_map for m in self.methods]
        names = ("vel", "x") + (("f", "var", "dvar") if variance_gain is not None else ())
        if variance_gain is not None:
            solver = dict(solver, variance_gain=variance_gain)
        out = rollout(maps[:-1], dynamics, starts, n_steps, affine, dt=dt, x0=x0, outputs=names if return_info else (), **solver)
        if self.verbose:
            status, done = out["status"], out["steps_done"]
            counts = ", ".join(f"{name} {int(np.sum(status == code))}" for code, name in enumerate(_lib.INV_STATUS_NAMES))
            print(f"Rollout of {len(done)} paths, {int(n_steps)} steps: {int(np.sum(done == int(n_steps)))} complete; last status: {counts}")
        return (out["path"], {k: v for k, v in out.items() if k != "path"}) if return_info else out["path"]

    def _still_dynamics(self):
        """A dynamics model for inverse_transport(), which asks the device call for x alone: zero velocities on two points,
        fitted once on the device of the last map."""
        if getattr(self, "_still", None) is None:
            from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
            from .gaussian_process import GaussianProcess
            D = self.n_features
            gp = GaussianProcess(kernel=ConstantKernel(1.0) * RBF(length_scale=[1.0] * D) + WhiteKernel(1e-6), optimizer=None,
                                 device=self.methods[-1].delta_map.device, verbose=False)
            self._still = gp.fit(np.vstack([np.zeros(D), np.ones(D)]), np.zeros((2, D)))
        return self._still

    def inverse_transport(self, points, x0=None, return_info=False, **solver):
        """The x with transport(x) = points: `x` of the same device call as transported_policy (with a dynamics of zero
        velocities, whose outputs are dropped).  With return_info also the status and the per-stage arrays."""
        out = self._pull(self._still_dynamics(), points, x0, False, solver, outputs=None if return_info else ("x",))
        info = {k: v for k, v in out.items() if k not in ("vel", "f", "x")}
        return (out["x"], info) if return_info else out["x"]

    def rollout_samples(self, dynamics, starts, n_steps, n_samples=10, dt=1.0, nugget=None, random_state=0, normals=None, x0=None,
                        return_info=False, **solver):
        """Which paths does the dynamics GP consider plausible from `starts` (M,D) of the LAST scene?  n_samples paths per start,
        each the rollout() of ONE function drawn from the posterior of `dynamics`, the draw of a step conditioned on the path's
        own earlier draws, in one device call (GaussianProcess.rollout_chain_samples: nugget, normals, random_state).  Only the
        dynamics is sampled; the maps act through their means.  Returns paths (M,n_samples,n_steps+1,D); with return_info also a
        dict: vel, x, f, pvar, cvar, steps_done, status (and chol for return_info="chol"), each with the leading shape
        (M,n_samples).  Zero normals give rollout()."""
        unknown = set(solver) - {"rtol", "max_passes"}
        if unknown:
            raise TypeError(f"TransportChain: unknown solver arguments {sorted(unknown)}")
        rollout = getattr(self.methods[-1].delta_map, "rollout_chain_samples", None)
        if rollout is None:
            raise NotImplementedError(f"TransportChain.rollout_samples(): the delta_map of the last transport ({type(self.methods[-1].delta_map).__name__}) "
                                      "has no rollout_chain_samples; GaussianProcess provides one")
        affine = [(m.affine_transform.rotation_matrix, m.affine_transform.scale, m.affine_transform.S_centroid,
                   m.affine_transform.T_centroid, m.affine_transform.rotation_matrix) for m in self.methods]
        maps = [m.delta_map for m in self.methods]
        out = rollout(maps[:-1], dynamics, starts, n_steps, affine, n_samples=n_samples, dt=dt, nugget=nugget, random_state=random_state,
                      normals=normals, x0=x0, return_info=return_info, **solver)
        if self.verbose:
            status, done = out["status"], out["steps_done"]
            counts = ", ".join(f"{name} {int(np.sum(status == code))}" for code, name in enumerate(_lib.ROLLOUT_SAMPLED_STATUS_NAMES))
            print(f"Sampled rollout of {done.size} paths, {int(n_steps)} steps: {int(np.sum(done == int(n_steps)))} complete; last status: {counts}")
        return (out["path"], {k: v for k, v in out.items() if k != "path"}) if return_info else out["path"]

    def rollout_functions(self, functions, starts, n_steps, dt=1.0, x0=None, return_info=False, **solver):
        """Where does the same plausible policy take the robot from all the `starts` (M,D) of the LAST scene?  The rollout() of
        every function of `functions` (GaussianProcess.sample_functions() of the dynamics: whole functions drawn from its
        posterior) from every start, all starts under the same functions, any number of steps, in one device call
        (GaussianProcess.rollout_chain_functions).  Only the dynamics is sampled; the maps act through their means.  Returns paths
        (M,S,n_steps+1,D); with return_info also a dict: vel, x, f, steps_done, status, each with the leading shape (M,S).
        Functions drawn with zero draws give rollout()."""
        unknown = set(solver) - {"rtol", "max_passes"}
        if unknown:
            raise TypeError(f"TransportChain: unknown solver arguments {sorted(unknown)}")
        rollout = getattr(self.methods[-1].delta_map, "rollout_chain_functions", None)
        if rollout is None:
            raise NotImplementedError(f"TransportChain.rollout_functions(): the delta_map of the last transport ({type(self.methods[-1].delta_map).__name__}) "
                                      "has no rollout_chain_functions; GaussianProcess provides one")
        affine = [(m.affine_transform.rotation_matrix, m.affine_transform.scale, m.affine_transform.S_centroid,
                   m.affine_transform.T_centroid, m.affine_transform.rotation_matrix) for m in self.methods]
        maps = [m.delta_map for m in self.methods]
        out = rollout(maps[:-1], functions, starts, n_steps, affine, dt=dt, x0=x0, return_info=return_info, **solver)
        if self.verbose:
            status, done = out["status"], out["steps_done"]
            counts = ", ".join(f"{name} {int(np.sum(status == code))}" for code, name in enumerate(_lib.INV_STATUS_NAMES))
            print(f"Rollout of {done.size} paths of drawn functions, {int(n_steps)} steps: {int(np.sum(done == int(n_steps)))} complete; last status: {counts}")
        return (out["path"], {k: v for k, v in out.items() if k != "path"}) if return_info else out["path"]
