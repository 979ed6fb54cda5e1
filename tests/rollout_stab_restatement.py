"""numpy restatement of the variance-stabilised rollout (csrc/gpt_rollout_stab.h, gpt_rollout_stabilised of include/gpt_hip.h).
Not a test; imported by tests/test_rollout_stabilised_cpu.py, tests/test_rollout_stabilised.py and tools.

One stabilised step, from the source-space quantities of a point (f its dynamics mean, var and dvar the posterior variance of the
dynamics and its gradient there):
    s    = sqrt(var) - std_offset
    ghat = dvar / |dvar|, the norm taken after scaling by max_d |dvar_d|; 0 where every dvar_d is exactly 0
    fs   = f - ((gain * s) * ghat)           each operation rounded on its own, as numpy rounds them
and vel = fs pushed through the maps as f is (tests/chain_restatement), y_{t+1} = y_t + dt * vel_t.  The loop, its end rule and
its NaN filling are tests/rollout_restatement.rollout: `stab_step` wraps a step of that module.

`variance_terms` is the fp64 algebra of the library for var and dvar (tests/posterior_restatement.posterior_float64's, with the
norms |V|, |V_d| kept): the reference values of the CPU tests and the SCALES of the tolerances of the GPU tests."""
import numpy as np

from tests import posterior_restatement as PR
from tests import rollout_restatement as RO

EPS = 2.0 ** -52
# The bound tests/test_input_ranges.py holds the variance launches to against the longdouble restatement, at its floor: MARGIN x
# FLOOR_ULPS ulps of the scale (tests/posterior_restatement.py).  The stabilised rollout's var and dvar are held to it against the
# merged launch at the same points.
PAIR_TOL = PR.MARGIN * PR.FLOOR_ULPS * EPS


def unit_gradient(g):
    """ghat (M,D) of g (M,D): csrc/gpt_rollout_stab.h unit_gradient, row by row."""
    g = np.asarray(g, dtype=np.float64)
    gmax = np.zeros(len(g))
    for d in range(g.shape[1]):
        gmax = np.fmax(gmax, np.abs(g[:, d]))
    zero = np.all(g == 0.0, axis=1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        h = g / gmax[:, None]
        n2 = h[:, 0] * h[:, 0]
        for d in range(1, g.shape[1]):
            n2 = n2 + h[:, d] * h[:, d]
        ghat = h / np.sqrt(n2)[:, None]
    ghat[zero] = 0.0
    return ghat


def stabilised(f, var, dvar, gain, std_offset):
    """fs (M,D) = f - ((gain * s) * ghat)."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.sqrt(np.asarray(var, dtype=np.float64)) - std_offset
        p = gain * s
        q = p[:, None] * unit_gradient(dvar)
        return np.asarray(f, dtype=np.float64) - q


def variance_terms(X, c, ls, noise, jitter, kind, Xq):
    """{var (M,), dvar (M,D), scale_var (M,), scale_dvar (M,D)} at the queries Xq of the model fitted on X: the library's algebra in
    fp64 numpy (W = L^-1 explicit, coordinates carrying 1 / sqrt2), scale_var = c + noise and scale_dvar = 2 |V| |V_d| as
    tests/posterior_restatement.SCALES names them."""
    X, Xq = np.asarray(X, dtype=np.float64), np.asarray(Xq, dtype=np.float64)
    N, D = X.shape
    inv = 1.0 / PR._full_ls(ls, D)
    Xs = X * inv
    a2, _ = PR._sq(Xs, Xs)
    k = PR.shapes(a2, kind, np.float64)[0]
    K = c * k
    K[np.diag_indices_from(K)] += noise + jitter
    W = np.linalg.inv(np.linalg.cholesky(K))
    hq, dq = PR._sq(Xq * (inv * PR.RS2), Xs * PR.RS2)
    ks, cg = PR.shapes(hq + hq, kind, np.float64, lnc=np.log(c))[:2]
    V = W @ ks.T
    nV = np.sqrt((V * V).sum(0))
    var = np.maximum((c + noise) - (V * V).sum(0), 0.0)
    dvar, sdv = np.zeros((len(Xq), D)), np.zeros((len(Xq), D))
    for d in range(D):
        Vd = W @ (cg * dq[d] * (inv[d] * PR.S2)).T
        dvar[:, d] = -2.0 * (Vd * V).sum(0)
        sdv[:, d] = 2.0 * nV * np.sqrt((Vd * Vd).sum(0))
    return {"var": var, "dvar": dvar, "scale_var": np.full(len(Xq), c + noise), "scale_dvar": sdv}


def stab_step(inner_step, source_terms, push, gain, std_offset):
    """A step of tests/rollout_restatement.rollout with the stabiliser: inner_step(y, guess) -> (x, f, status) is the mean step
    with f the SOURCE-space mean; source_terms(x) -> (var (m,), dvar (m,D)); push(x, v, y, guess) -> the vector v pushed through
    the maps at x (the identity without maps).  Records f, var, dvar of every call in the lists of its `seen` attribute."""
    def step(y, guess):
        x, f, status = inner_step(y, guess)
        var, dvar = source_terms(x)
        vel = push(x, stabilised(f, var, dvar, gain, std_offset), y, guess)
        step.seen.append((np.asarray(f), np.asarray(var), np.asarray(dvar)))
        return x, vel, status
    step.seen = []
    return step


def rollout(step, y0, n_steps, dt=1.0, x0=None):
    """tests/rollout_restatement.rollout: the loop, the end rule and the NaN filling are the mean rollout's."""
    return RO.rollout(step, y0, n_steps, dt=dt, x0=x0)
