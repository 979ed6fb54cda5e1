"""Whole functions drawn from the posterior of a fitted GaussianProcess, by pathwise conditioning (Matheron's rule): draw the prior
function as a finite sum of random Fourier features, correct it with one solve against the training data, and what is left is an
ordinary deterministic function

    F_s(x) = k(x, X) V_s + sum_j ( a_sj cos(omega_j . x) + b_sj sin(omega_j . x) ),
    V_s    = (K + sigma^2 I)^-1 (Y - prior_s(X) - sigma eps_s)

that can be evaluated anywhere, for any number of steps, from any number of starts (the device call: _lib.Handle.rollout_pathwise;
the solve: _lib.Handle.apply_inverse).  The approximation is in the prior only, its covariance error falling as 1 / sqrt(J); the
update against the data is exact, and the mean of the drawn functions is the posterior mean exactly.  The reference draws joint
samples at fixed points only (GaussianProcess.samples); GaussianProcess.rollout_samples is the exact call for short paths, each path
a function of its own.

The three helpers at the top are pure numpy and need no GPU."""
from __future__ import annotations

import numpy as np

_KERNEL_NU = {0: None, 2: 1.5, 3: 2.5, "rbf": None, "matern32": 1.5, "matern52": 2.5}


def draw_frequencies(kernel_type, length_scale, J, rs):
    """J frequencies (J,D) of the spectral density of the stationary kernel: kernel_type the GPT_KERNEL_* code of
    gaussian_process.kernel_type (0 RBF, 2 Matern 3/2, 3 Matern 5/2) or "rbf" / "matern32" / "matern52"; length_scale (D,); rs a
    np.random.RandomState.  RBF: omega = z / l with z = rs.standard_normal((J, D)).  Matern nu: the same z, then
    g = rs.chisquare(2 nu, J) and omega = (z / l) sqrt(2 nu / g) (a Student-t with 2 nu degrees of freedom).  Matern 1/2 is refused:
    its Cauchy frequencies do not converge usefully."""
    if kernel_type in (1, "matern12"):
        raise ValueError("draw_frequencies: Matern(nu=0.5) has Cauchy-distributed frequencies, whose feature sum does not converge "
                         "usefully; RBF, Matern 3/2 or Matern 5/2")
    if kernel_type not in _KERNEL_NU:
        raise ValueError(f"draw_frequencies: unknown kernel_type {kernel_type!r}")
    ls = np.asarray(length_scale, dtype=np.float64)
    if ls.ndim != 1 or ls.size < 1 or not np.all(ls > 0) or not np.all(np.isfinite(ls)):
        raise ValueError(f"draw_frequencies: length_scale must be a (D,) array of positive numbers, got {length_scale!r}")
    if int(J) != J or int(J) < 0:
        raise ValueError(f"draw_frequencies: J must be an integer >= 0, got {J!r}")
    J = int(J)
    omega = rs.standard_normal((J, ls.size)) / ls
    nu = _KERNEL_NU[kernel_type]
    if nu is not None:
        g = rs.chisquare(2.0 * nu, J)
        omega = omega * np.sqrt(2.0 * nu / g)[:, None]
    return np.ascontiguousarray(omega)


def draw_amplitudes(c, J, S, O, rs):
    """The amplitudes (S,J,2,O) of S prior functions with O outputs over J frequencies, prior variance c: sqrt(c / J) times
    rs.standard_normal((S, J, 2, O)); [:, :, 0] multiplies the cosines, [:, :, 1] the sines."""
    if not float(c) > 0.0:
        raise ValueError(f"draw_amplitudes: c must be > 0, got {c!r}")
    for name, v, low in (("J", J, 0), ("S", S, 1), ("O", O, 1)):
        if int(v) != v or int(v) < low:
            raise ValueError(f"draw_amplitudes: {name} must be an integer >= {low}, got {v!r}")
    w = rs.standard_normal((int(S), int(J), 2, int(O)))
    return w * np.sqrt(float(c) / int(J)) if int(J) else w


def prior_at(X, omega, amp):
    """The prior functions at the points X (N,D): (S,N,O), sum_j amp[s,j,0] cos(omega_j . x) + amp[s,j,1] sin(omega_j . x)."""
    X, omega, amp = np.asarray(X, dtype=np.float64), np.asarray(omega, dtype=np.float64), np.asarray(amp, dtype=np.float64)
    if X.ndim != 2 or omega.ndim != 2 or omega.shape[1] != X.shape[1]:
        raise ValueError(f"prior_at: X has shape {X.shape} and omega {omega.shape}, expected (N, D) and (J, D)")
    if amp.ndim != 4 or amp.shape[1] != omega.shape[0] or amp.shape[2] != 2:
        raise ValueError(f"prior_at: amp has shape {amp.shape}, expected (S, J, 2, O) with J = {omega.shape[0]}")
    theta = X @ omega.T
    return np.einsum("nj,sjo->sno", np.cos(theta), amp[:, :, 0]) + np.einsum("nj,sjo->sno", np.sin(theta), amp[:, :, 1])


def sample_functions(gp, n_functions=10, n_frequencies=2048, random_state=0, frequencies=None, draws=None):
    """GaussianProcess.sample_functions: see there."""
    from . import _lib
    gp._check_chain("sample_functions", [], gp, [], 0)
    if gp._ktype == 1:
        raise NotImplementedError("sample_functions(): Matern(nu=0.5) has Cauchy-distributed frequencies, whose feature sum does not "
                                  "converge usefully; rollout_samples() draws from such a model exactly")
    X, Y = gp.X, gp.Y
    N, D = X.shape
    O = Y.shape[1]
    ls = np.broadcast_to(np.asarray(gp._ls, dtype=np.float64), (D,))
    rs = np.random.RandomState(random_state)
    if frequencies is None:
        omega = draw_frequencies(gp._ktype, ls, n_frequencies, rs)
    else:
        omega = _lib.as_f64(frequencies, 2, "frequencies")
        if omega.shape[1] != D:
            raise ValueError(f"sample_functions(): frequencies has shape {omega.shape}, expected (J, {D})")
    J = omega.shape[0]
    if J > _lib.PATHWISE_MAX_FREQ:
        raise ValueError(f"sample_functions(): at most {_lib.PATHWISE_MAX_FREQ} (_lib.PATHWISE_MAX_FREQ) frequencies, got {J}")
    if draws is None:
        if int(n_functions) != n_functions or int(n_functions) < 1:
            raise ValueError(f"sample_functions(): n_functions must be an integer >= 1, got {n_functions!r}")
        S = int(n_functions)
        amp = draw_amplitudes(gp._c, J, S, O, rs)
        eps = rs.standard_normal((S, N, O))
    else:
        w, eps = (_lib.as_f64(a, n, name) for a, n, name in zip(draws, (4, 3), ("draws[0]", "draws[1]")))
        S = w.shape[0]
        if S < 1 or w.shape != (S, J, 2, O) or eps.shape != (S, N, O):
            raise ValueError(f"sample_functions(): draws has shapes {w.shape} and {eps.shape}, expected (S, {J}, 2, {O}) and (S, {N}, {O})")
        amp = w * np.sqrt(gp._c / J) if J else w
    R = Y[None] - prior_at(X, omega, amp) - np.sqrt(gp.noise_var_) * eps
    handle = getattr(gp._handle, "primary", gp._handle)
    V = handle.apply_inverse(np.ascontiguousarray(R.transpose(1, 0, 2).reshape(N, S * O)))
    weights = np.ascontiguousarray(V.reshape(N, S, O).transpose(1, 0, 2))
    return PosteriorFunctions(gp, omega, np.ascontiguousarray(amp), weights)


class PosteriorFunctions:
    """S functions drawn from the posterior of the fitted GaussianProcess `gp` (GaussianProcess.sample_functions): omega (J,D) the
    frequencies they share, amplitudes (S,J,2,O) and weights (S,N,O) = the V_s.  They belong to the fit they were drawn from."""

    def __init__(self, gp, omega, amplitudes, weights, fit_token=None):
        self.gp = gp
        self._fit_token = getattr(gp, "_fit_token", None) if fit_token is None else fit_token      # the fit the draws belong to
        self.omega = omega
        self.amplitudes = amplitudes
        self.weights = weights

    def __len__(self):
        return self.weights.shape[0]

    def subset(self, idx):
        """The functions idx (indices, a slice or a mask) as a PosteriorFunctions of their own; the frequencies are shared."""
        idx = np.arange(len(self))[idx].reshape(-1)
        if idx.size < 1:
            raise IndexError("PosteriorFunctions.subset(): no function selected")
        return PosteriorFunctions(self.gp, self.omega, np.ascontiguousarray(self.amplitudes[idx]), np.ascontiguousarray(self.weights[idx]),
                                  self._fit_token)

    def _call(self, what, maps, affine, y0, func, n_steps, dt, x0, rtol, max_passes, outputs):
        gp = self.gp
        gp._require_fit()
        if getattr(gp, "_fit_token", None) is not self._fit_token or self.weights.shape[1:] != (len(gp.X), gp.n_outputs):
            raise RuntimeError(f"{what}(): the model has been fitted again since these functions were drawn")
        primary = lambda g: getattr(g._handle, "primary", g._handle)
        stages = [(primary(g), rot, src, dst, scale, jac) for g, (rot, scale, src, dst, jac) in zip(maps, affine)]
        owner = primary(maps[-1]) if maps else primary(gp)
        return owner.rollout_pathwise(stages, primary(gp), y0, func, self.weights, self.omega, self.amplitudes, int(n_steps), dt=float(dt), x0=x0,
                                      rtol=rtol, max_passes=max_passes, outputs=outputs)

    def predict(self, x):
        """The functions at the points x (M,D): (S,M,O), from one step of the device call at x."""
        x, _ = self.gp._check_chain_points("PosteriorFunctions.predict", x, None, 1e-10, 64, "x")
        S, M = len(self), x.shape[0]
        out = self._call("PosteriorFunctions.predict", [], [], np.tile(x, (S, 1)), np.repeat(np.arange(S), M), 1, 1.0, None, 1e-10, 64, ("f",))
        return out["f"][:, 0].reshape(S, M, -1)

    def _rollout(self, what, maps, affine, starts, n_steps, dt, x0, rtol, max_passes, return_info):
        starts, x0 = self.gp._check_chain_points(what, starts, x0, rtol, max_passes, "starts")
        if int(n_steps) != n_steps or int(n_steps) < 0:
            raise ValueError(f"{what}(): n_steps must be an integer >= 0, got {n_steps!r}")
        if not np.isfinite(float(dt)) or float(dt) == 0.0:
            raise ValueError(f"{what}(): dt must be finite and not zero, got {dt!r}")
        M, S, T = starts.shape[0], len(self), int(n_steps)
        if M * S * (T + 1) >= 2 ** 31:
            raise ValueError(f"{what}(): starts times functions times (n_steps + 1), the rows of the paths, must stay below 2^31")
        out = self._call(what, maps, affine, np.repeat(starts, S, axis=0), np.tile(np.arange(S), M), T, dt,
                         None if x0 is None else np.repeat(x0, S, axis=0), rtol, max_passes, ("vel", "x", "f") if return_info else ())
        return {k: v.reshape((M, S) + v.shape[1:]) for k, v in out.items()}       # path index = m * S + j

    def rollout(self, starts, n_steps, dt=1.0, return_info=False):
        """The paths of every function from every row of `starts` (M,D), all starts under the same functions: n_steps explicit Euler
        steps y_{t+1} = y_t + dt * F_s(y_t), the loop over the steps on the device in one call.  Returns paths (M,S,n_steps+1,D),
        path index m * S + j as GaussianProcess.rollout_samples; with return_info also a dict: vel, x, f (M,S,n_steps,D),
        steps_done and status (M,S).  A path ends where its next point is not finite; the rows after that are NaN."""
        out = self._rollout("PosteriorFunctions.rollout", [], [], starts, n_steps, dt, None, 1e-10, 64, return_info)
        return (out["path"], {k: v for k, v in out.items() if k != "path"}) if return_info else out["path"]
