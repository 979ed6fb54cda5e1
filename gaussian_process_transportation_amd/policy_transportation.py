"""PolicyTransportation — Phi(x) = gamma(x) + Psi(gamma(x)) with gamma an AffineTransform and Psi
any `delta_map` exposing fit / predict / derivative / samples (duck-typed plugin slot of the
reference, policy_transportation/transportation/policy_transportation.py:11-84); `inverse_transport` (an addition) needs a
delta_map that also has `invert_displacement`, `transport_all` one with `transport_policy`, `transported_policy` one with
`pullback_policy`."""
import numpy as np

from .affine_transform import AffineTransform


class PolicyTransportation:
    def __init__(self, method, verbose=True):
        self.delta_map = method
        self.verbose = verbose

    def fit(self, source_distribution, target_distribution, do_scale=False, do_rotation=True):
        self.affine_transform = AffineTransform(do_scale=do_scale, do_rotation=do_rotation, verbose=self.verbose)
        self.affine_transform.fit(source_distribution, target_distribution)
        source_aligned = self.affine_transform.predict(source_distribution)
        self.delta_distribution = np.asarray(target_distribution, dtype=np.float64) - source_aligned
        self.delta_map.fit(source_aligned, self.delta_distribution)

    def prefetch(self, pos):
        """Optional: lets a delta_map that can (GaussianProcess.prefetch_posterior) compute what transport(pos) and
        transport_velocity(pos, .) will ask for in one pass.  No effect on results."""
        hook = getattr(self.delta_map, "prefetch_posterior", None)
        if hook is None:
            return
        try:
            hook(self.affine_transform.predict(pos))
        except NotImplementedError:            # e.g. a Matern delta_map: the calls that follow decide what fails
            pass

    def transport(self, pos, return_std=True):
        """Returns (transported positions, std).  The reference raises NameError for
        return_std=False (its :35 returns an unbound name); here std is None in that case."""
        pos_rotated = self.affine_transform.predict(pos)
        if return_std:
            delta_mean, delta_std = self.delta_map.predict(pos_rotated, return_std=True)
        else:
            delta_mean, delta_std = self.delta_map.predict(pos_rotated, return_std=False), None
        return pos_rotated + delta_mean, delta_std

    def inverse_transport(self, pos, x0=None, return_info=False, **solver):
        """The x with transport(x) = pos: Phi^-1 = gamma^-1 o (id + Psi)^-1.  The displacement part is solved by the
        delta_map (`invert_displacement`, e.g. GaussianProcess: damped Newton on the device; `solver` passes rtol /
        max_passes on), started at gamma(x0) when x0 (a guess of the preimage) is given; the affine part is closed form.
        With return_info also the delta_map's dict (status, passes, residual, det per point).  The reference has no inverse:
        its inverse-mapping example (example/2D/surface_generalization_heteroschedastic _inverse_mapping.py:88-127) fits a
        second transport backwards instead."""
        invert = getattr(self.delta_map, "invert_displacement", None)
        if invert is None:
            raise NotImplementedError(f"inverse_transport(): the delta_map ({type(self.delta_map).__name__}) has no "
                                      "invert_displacement(y, x0, ..., return_info=True); GaussianProcess provides one")
        z0 = None if x0 is None else self.affine_transform.predict(x0)
        z, info = invert(np.asarray(pos, dtype=np.float64), z0, return_info=True, **solver)
        if self.verbose:
            from ._lib import INV_CONVERGED, INV_STATUS_NAMES
            status = np.asarray(info["status"])
            counts = ", ".join(f"{name} {int(np.sum(status == code))}" for code, name in enumerate(INV_STATUS_NAMES))
            solved = status == INV_CONVERGED
            print(f"Inverse of the map: {counts}; det(I + J_psi) <= 0 at {int(np.sum(np.asarray(info['det'])[solved] <= 0))} "
                  f"of {int(np.sum(solved))} solutions (the map folds there: not a diffeomorphism)")
        x = self.affine_transform.inverse_predict(z)
        return (x, info) if return_info else x

    def transport_velocity(self, pos, vel, return_var=True):
        """Push velocities through the Jacobian of Phi; variance from the Jacobian variance (:37-59)."""
        pos_rotated = self.affine_transform.predict(pos)
        J_gamma = self.affine_transform.derivative(pos)
        if return_var:
            J_psi, J_psi_var = self.delta_map.derivative(pos_rotated, return_var=True)
        else:
            J_psi, J_psi_var = self.delta_map.derivative(pos_rotated, return_var=False), None
        J_phi = J_gamma + J_psi @ J_gamma
        if self.verbose:
            print("Is the map locally diffeomorphic?", np.all(np.abs(np.linalg.det(J_phi)) > 0))
        vel = np.asarray(vel, dtype=np.float64)[:, :, None]
        vel_rotated = J_gamma @ vel
        vel_transported = (J_phi @ vel)[:, :, 0]
        if J_psi_var is None:
            return vel_transported, None
        var_vel_transported = (J_psi_var @ vel_rotated ** 2)[:, :, 0]
        return vel_transported, var_vel_transported

    def transport_orientation(self, pos, ori):
        """Rotate orientations (w,x,y,z quaternions) by the rotation closest to J_Phi, evaluated — as
        the reference does (:62) — at the UN-rotated positions."""
        from .quaternion import quaternion_from_nonorthogonal, quaternion_multiply
        J_phi = self.delta_map.derivative(pos)
        J_gamma = self.affine_transform.derivative(pos)
        J_phi = J_gamma + J_phi @ J_gamma
        if self.verbose:
            print("Is the map locally diffeomorphic?", np.all(np.linalg.det(J_phi) > 0))
        if J_phi[0].shape[0] != 3:
            print("The Jacobain of the map as shape ", J_phi[0].shape, " but it should be (3x3)")
            print("Robot orientation is not transported")
            return None
        return quaternion_multiply(quaternion_from_nonorthogonal(J_phi), np.asarray(ori, dtype=np.float64))

    def transport_all(self, pos, vel=None, ori=None, return_info=False):
        """transport(pos), transport_velocity(pos, vel) and transport_orientation(pos, ori) in ONE call of the delta_map's
        `transport_policy` (GaussianProcess: the affine part, the posterior and this file's algebra on the device).  Returns
        (positions, std, velocities, velocity variance, orientations), None for what was not given — and for orientations
        when the space is not 3-D, after the reference's two lines.  With return_info also the delta_map's dict (det_vel,
        det_ori, ori_gap, pos_rot per point).  Velocities use the reference's unscaled Jacobian of the affine part
        (AffineTransform.derivative); orientations its Jacobian at the UN-rotated positions (transport_orientation)."""
        fused = getattr(self.delta_map, "transport_policy", None)
        if fused is None:
            raise NotImplementedError(f"transport_all(): the delta_map ({type(self.delta_map).__name__}) has no "
                                      "transport_policy(x, rotation, scale, source_centroid, target_centroid, ...); "
                                      "GaussianProcess provides one")
        aff = self.affine_transform
        out = fused(pos, aff.rotation_matrix, aff.scale, aff.S_centroid, aff.T_centroid, jacobian=aff.rotation_matrix, vel=vel, ori=ori)
        if vel is not None and self.verbose:
            print("Is the map locally diffeomorphic?", np.all(np.abs(out["det_vel"]) > 0))
        ori_out = None
        if ori is not None:
            if self.verbose:
                print("Is the map locally diffeomorphic?", np.all(out["det_ori"] > 0))
            D = np.shape(aff.rotation_matrix)[0]
            if D != 3:
                print("The Jacobain of the map as shape ", (D, D), " but it should be (3x3)")
                print("Robot orientation is not transported")
            else:
                ori_out = out["ori"]
        res = (out["pos"], out["std"], out.get("vel"), out.get("vel_var"), ori_out)
        return res + (out,) if return_info else res

    def transported_policy(self, dynamics, pos, x0=None, return_std=False, return_info=False, **solver):
        """The transported policy at points `pos` (M,D) of the target scene that need not lie on the demonstration: the
        velocity J_Phi(x) dynamics.predict(x) at x = inverse_transport(pos), `dynamics` a GaussianProcess fitted on the source
        demonstration — in ONE call of the delta_map's `pullback_policy` (GaussianProcess: inverse, dynamics and push-forward
        in one launch on the device), where the reference refits a GP on the moved demonstration
        (example/2D/surface_generalization.py:81-88).  x0: a guess of the preimages; `solver` passes rtol / max_passes on.
        Returns the velocities (M,D); with return_std also std (M,D) = sqrt(vel_var_dyn + vel_var_map), the sum of the
        dynamics' own uncertainty pushed through J_Phi and of the map's (transport_velocity's variance), the two parts the
        reference's heteroscedastic example adds up; with return_info also a dict: x, status, passes, residual, det, f and
        (return_std) std_dyn, vel_var_dyn, vel_var_map, map_std per point.  Velocities use the reference's unscaled Jacobian
        of the affine part (AffineTransform.derivative), as transport_velocity does."""
        pull = getattr(self.delta_map, "pullback_policy", None)
        if pull is None:
            raise NotImplementedError(f"transported_policy(): the delta_map ({type(self.delta_map).__name__}) has no "
                                      "pullback_policy(dynamics, y, rotation, scale, source_centroid, target_centroid, ...); "
                                      "GaussianProcess provides one")
        aff = self.affine_transform
        out = pull(dynamics, np.asarray(pos, dtype=np.float64), aff.rotation_matrix, aff.scale, aff.S_centroid, aff.T_centroid,
                   jacobian=aff.rotation_matrix, x0=x0, variances=(True if return_info else "vel") if return_std else False, **solver)
        if self.verbose:
            from ._lib import INV_CONVERGED, INV_STATUS_NAMES
            status = np.asarray(out["status"])
            counts = ", ".join(f"{name} {int(np.sum(status == code))}" for code, name in enumerate(INV_STATUS_NAMES))
            solved = status == INV_CONVERGED
            print(f"Inverse of the map: {counts}; det(I + J_psi) <= 0 at {int(np.sum(np.asarray(out['det'])[solved] <= 0))} "
                  f"of {int(np.sum(solved))} solutions (the map folds there: not a diffeomorphism)")
        res = (out["vel"],)
        if return_std:
            res += (np.sqrt(out["vel_var_dyn"] + out["vel_var_map"]),)
        if return_info:
            res += ({k: v for k, v in out.items() if k != "vel"},)
        return res if len(res) > 1 else res[0]

    def rollout_policy(self, dynamics, starts, n_steps, dt=1.0, x0=None, return_info=False, variance_gain=None, **solver):
        """The paths transported_policy() drives from `starts` (M,D) of the target scene: n_steps explicit Euler steps
        y += dt * transported_policy(dynamics, y), the loop over the steps on the device in one call
        (TransportChain.rollout with this transport as its only stage).  Returns path (M,n_steps+1,D); with return_info also a
        dict: vel, x, steps_done, status."""
        from .transport_chain import TransportChain
        return TransportChain([self], verbose=self.verbose).rollout(dynamics, starts, n_steps, dt=dt, x0=x0, return_info=return_info,
                                                                variance_gain=variance_gain, **solver)

    def rollout_policy_samples(self, dynamics, starts, n_steps, n_samples=10, dt=1.0, nugget=None, random_state=0, normals=None,
                               x0=None, return_info=False, **solver):
        """n_samples paths per start of rollout_policy() when the dynamics is a function drawn from the posterior of `dynamics`
        (TransportChain.rollout_samples with this transport as its only stage).  Only the dynamics is sampled; the map acts
        through its mean.  Returns paths (M,n_samples,n_steps+1,D); with return_info also a dict."""
        from .transport_chain import TransportChain
        return TransportChain([self], verbose=self.verbose).rollout_samples(dynamics, starts, n_steps, n_samples=n_samples, dt=dt,
                                                                        nugget=nugget, random_state=random_state, normals=normals, x0=x0,
                                                                        return_info=return_info, **solver)

    def rollout_policy_functions(self, functions, starts, n_steps, dt=1.0, x0=None, return_info=False, **solver):
        """The paths of rollout_policy() from every start under each of `functions`, whole functions drawn from the posterior of the
        dynamics (GaussianProcess.sample_functions; TransportChain.rollout_functions with this transport as its only stage).  Only
        the dynamics is sampled; the map acts through its mean.  Returns paths (M,S,n_steps+1,D); with return_info also a dict."""
        from .transport_chain import TransportChain
        return TransportChain([self], verbose=self.verbose).rollout_functions(functions, starts, n_steps, dt=dt, x0=x0, return_info=return_info,
                                                                          **solver)

    def sample_transportation(self, pos):
        pos_rotated = self.affine_transform.predict(pos)
        return pos_rotated + self.delta_map.samples(pos_rotated)
