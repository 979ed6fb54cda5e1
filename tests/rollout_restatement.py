"""numpy restatement of a rollout of the transported policy (csrc/gpt_rollout.hip, gpt_rollout_policy of include/gpt_hip.h).  Not
a test; imported by tests/test_policy_rollout.py, examples and tools.

`rollout` is the definition around ANY evaluation of one step: per trajectory, for t = 0 .. T-1,
    (x_t, vel_t, status_t) = step(y_t, guess),   guess = x_{t-1} (at t = 0: x0, or None),
    y_{t+1} = y_t + dt * vel_t   (numpy: the product and the sum rounded separately),
and the trajectory ENDS at the first t where status_t is not CONVERGED or y_{t+1} is not finite: x_t, vel_t and status_t are still
recorded, y_{t+1} is not, and every row after the end is NaN.  `step` sees all trajectories still alive at once, (m,D) arrays, and
returns (x (m,D), vel (m,D), status (m,)); tests/test_policy_rollout.py passes the existing device call
(TransportChain.transported_policy) there, which makes this loop the host loop the device call replaces.

`chain_step` is the step restated in numpy: tests/chain_restatement.chain at the points given.  `mean_step` is the step of a
rollout without maps: x = y, vel = the mean of the dynamics."""
import numpy as np

from tests import chain_restatement as CH
from tests import inverse_map_restatement as INV


def chain_step(models, dyn_model, affs, rtol=1e-10, max_passes=64):
    """step(y, guess) through tests/chain_restatement.chain."""
    def step(y, guess):
        out = CH.chain(models, dyn_model, affs, y, x0=guess, rtol=rtol, max_passes=max_passes)
        return out["x"], out["vel"], out["status"]
    return step


def mean_step(dyn_model):
    def step(y, guess):
        return y.copy(), dyn_model.mean(y)[0].astype(np.float64), np.full(len(y), INV.CONVERGED, dtype=np.int32)
    return step


def rollout(step, y0, n_steps, dt=1.0, x0=None):
    """{path (M,T+1,D), vel (M,T,D), x (M,T,D), steps_done (M,), status (M,)} of the definition above."""
    y0 = np.asarray(y0, dtype=np.float64)
    M, D = y0.shape
    T = int(n_steps)
    path, vel, x = np.full((M, T + 1, D), np.nan), np.full((M, T, D), np.nan), np.full((M, T, D), np.nan)
    steps_done, status = np.zeros(M, dtype=np.int32), np.full(M, INV.CONVERGED, dtype=np.int32)
    path[:, 0] = y0
    alive = np.arange(M)
    guess = None if x0 is None else np.asarray(x0, dtype=np.float64)
    for t in range(T):
        if len(alive) == 0:
            break
        xt, vt, st = step(np.ascontiguousarray(path[alive, t]), guess)
        x[alive, t], vel[alive, t], status[alive] = xt, vt, st
        with np.errstate(over="ignore", invalid="ignore"):
            nxt = path[alive, t] + dt * vt
        go = (np.asarray(st) == INV.CONVERGED) & np.all(np.isfinite(nxt), axis=1)
        steps_done[alive] = t + go
        path[alive[go], t + 1] = nxt[go]
        alive, guess = alive[go], np.ascontiguousarray(np.asarray(xt)[go])
    return {"path": path, "vel": vel, "x": x, "steps_done": steps_done, "status": status}
