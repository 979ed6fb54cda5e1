"""Whole paths of the variance-stabilised policy in one device call: gpt_rollout_stabilised (csrc/gpt_rollout_stab.hip: four
trajectories per workgroup, the product with the inverse factor on the matrix cores inside the step loop),
GaussianProcess.rollout / TransportChain.rollout / GaussianProcessTransportation.rollout_policy with variance_gain.

What holds the kernel:
  1. gain = 0 is the merged mean rollout, bit for bit (every line of the new body but the stabiliser's own).
  2. var_t and dvar_t against the merged variance launch (predict_all) at the device's own x_t, within the bound
     tests/test_input_ranges.py holds that launch to at its floor: MARGIN x FLOOR_ULPS = 16 x 64 ulps of the scale
     (rollout_stab_restatement.PAIR_TOL), scale = c + noise for var and 2 |V| |V_d| for dvar (posterior_restatement.SCALES),
     computed by the fp64 numpy restatement, never from the new kernel.  Both launches multiply the same packed factor by the
     same columns and add the N products in different orders.
  3. vel_t against the definition evaluated in numpy from the device's own f_t, var_t, dvar_t: 4 ulps of max(|f_t,d|, gain |s_t|)
     (K >= 1: of the largest of them times the 1-norm of the pushed matrix product), and path[t+1] == path[t] + dt * vel[t] bitwise.
  4. independence of M, neighbours, order and launch cuts, bit for bit.
Models as tests/test_policy_rollout.py: the letter-S map (20 points), the rings (36), the dynamics on the demonstration (400);
M = 9, T = 12 unless said otherwise."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import inverse_map_restatement as INV
from tests import rollout_stab_restatement as RS
from tests.conftest import load_golden
from tests.test_policy_rollout import M9, T12, _letter_starts, _sentinels, _stage_tuples
from tests.test_pullback_chain import _case, _fit_rings
from tests.test_pullback_policy import EPS, LD, RTOL, _fit_gp, _fit_transport, _untouched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN_NAMES = ("path", "vel", "x", "steps_done", "status")
ALL_NAMES = ("path", "vel", "x", "f", "var", "dvar", "steps_done", "status")
KIND = {None: "rbf", 1.5: "matern32", 2.5: "matern52"}


# ------------------------------------------------------------------------------------------------------------ helpers
def _stab(chain, dyn, y0, T, gain, dt=1.0, x0=None, **solver):
    """The device call through the public interface: chain None = the dynamics rolls out itself."""
    if chain is None:
        path, info = dyn.rollout(y0, T, dt=dt, return_info=True, variance_gain=gain)
    else:
        path, info = chain.rollout(dyn, y0, T, dt=dt, x0=x0, return_info=True, variance_gain=gain, **solver)
    return dict(info, path=path)


def _mean(chain, dyn, y0, T, dt=1.0, x0=None, **solver):
    if chain is None:
        path, info = dyn.rollout(y0, T, dt=dt, return_info=True)
    else:
        path, info = chain.rollout(dyn, y0, T, dt=dt, x0=x0, return_info=True, **solver)
    return dict(info, path=path)


def _same(got, want, what, names=ALL_NAMES):
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def _recorded(out):
    """(m, t) of every step the device recorded: t <= steps_done[m], t < T."""
    T = out["vel"].shape[1]
    return [(m, t) for m, done in enumerate(out["steps_done"]) for t in range(min(int(done) + 1, T))]


def _check_nan_layout(out):
    T = out["vel"].shape[1]
    for m, done in enumerate(out["steps_done"]):
        last = min(int(done) + 1, T)
        assert np.all(np.isfinite(out["path"][m, :done + 1])) and np.all(np.isnan(out["path"][m, done + 1:])), m
        for k in ("vel", "x", "f", "var", "dvar"):
            assert np.all(np.isnan(out[k][m, last:])), (k, m)
        for k in ("x", "f", "var"):
            assert np.all(np.isfinite(out[k][m, :last])), (k, m)


def _check_variance(out, gp, nu, what):
    """Check 2: var and dvar of every recorded step against the merged launch at the device's x_t."""
    rec = _recorded(out)
    xq = np.ascontiguousarray(np.stack([out["x"][m, t] for m, t in rec]))
    ref = gp._handle.predict_all(xq, var=True, dvar=True)
    sc = RS.variance_terms(gp.X, gp._c, gp._ls, gp._noise, gp.alpha, KIND[nu], xq)
    var = np.array([out["var"][m, t] for m, t in rec])
    dvar = np.stack([out["dvar"][m, t] for m, t in rec])
    e_var = np.abs(var - ref["var"].reshape(-1)) / sc["scale_var"]
    tol_d = RS.PAIR_TOL * sc["scale_dvar"] + (2 * gp.X.shape[0] + 2) * RS.PR.TINY
    e_dvar = np.abs(dvar - ref["dvar"].T)
    share_d = float(np.max(np.divide(e_dvar, tol_d, out=np.zeros_like(e_dvar), where=tol_d > 0)))
    print(f"{what}: {len(rec)} steps; var against the merged launch {float(e_var.max()) / RS.PAIR_TOL:.4f} of the bound "
          f"({float(e_var.max()) / EPS:.1f} ulps of c + noise), dvar {share_d:.4f} of the bound")
    assert np.all(e_var <= RS.PAIR_TOL), what
    assert np.all(e_dvar <= tol_d), what
    # and the fp64 restatement agrees with both at the level fp64 resolves these models (not the bound under test)
    assert np.all(np.abs(var - sc["var"]) <= 1e-6 * sc["scale_var"])


def _pushed(chain, dyn, out, m, t, fs, solver):
    """fs through the maps at step (m, t): Q (A_0 (R_jac,0 fs)) in longdouble from the per-stage A of transported_policy at y_t
    with the guess x_{t-1}, and the 1-norm of the matrix that is applied."""
    first = solver.get("x0_first")
    guess = out["x"][m, t - 1][None] if t > 0 else (None if first is None else first[m:m + 1])
    kw = {k: v for k, v in solver.items() if k != "x0_first"}
    _, info = chain.transported_policy(dyn, np.ascontiguousarray(out["path"][m, t][None]), x0=None if guess is None else np.ascontiguousarray(guess),
                                       return_info=True, **kw)
    assert_array_equal(info["x"][0], out["x"][m, t])
    A = info["stage_A"][:, 0].astype(LD)
    R = [np.asarray(mt.affine_transform.rotation_matrix, dtype=LD) for mt in chain.methods]
    v = A[0] @ (R[0] @ fs.astype(LD))
    P = A[0] @ R[0]
    Q = np.eye(len(fs), dtype=LD)
    for k in range(1, len(R)):
        Q = (A[k] @ R[k]) @ Q
    return (Q @ v).astype(np.float64), float(np.max(np.sum(np.abs(Q @ P), axis=0)))


def _check_velocity(out, gain, dt, off, what, chain=None, dyn=None, **solver):
    """Check 3."""
    worst = 0.0
    for m, t in _recorded(out):
        f, var, dvar = out["f"][m, t], out["var"][m, t], out["dvar"][m, t]
        fs = RS.stabilised(f[None], np.array([var]), dvar[None], gain, off)[0]
        s = np.sqrt(var) - off
        if chain is None:
            want, tol = fs, 4 * EPS * np.maximum(np.abs(f), gain * abs(s))
        else:
            want, norm = _pushed(chain, dyn, out, m, t, fs, solver)
            tol = 4 * EPS * max(np.max(np.abs(f)), gain * abs(s)) * norm
        fin = np.isfinite(want)
        assert_array_equal(np.isfinite(out["vel"][m, t]), fin, err_msg=f"{what} step {m},{t}: vel is finite where the definition is")
        err = np.abs(out["vel"][m, t] - want)[fin]
        if err.size:
            worst = max(worst, float(np.max(err / np.maximum(np.broadcast_to(tol, fin.shape)[fin], 1e-300))))
            assert np.all(err <= np.broadcast_to(tol, fin.shape)[fin]), (what, m, t, out["vel"][m, t], want, tol)
        if t < out["steps_done"][m]:
            assert_array_equal(out["path"][m, t + 1], out["path"][m, t] + dt * out["vel"][m, t], err_msg=f"{what} step {m},{t}")
    print(f"{what}: vel against the definition from the device's f, var, dvar: largest share of the bound {worst:.3f}")


@pytest.fixture(scope="module")
def letter2():
    from gaussian_process_transportation_amd import TransportChain
    g = load_golden("letterS_2d")
    tr0, tr1 = _fit_transport(g), _fit_rings(g["traj"][200])
    dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01)
    return dict(_case([tr0, tr1], dyn, [None, None]), g=g, chain=TransportChain([tr0, tr1], verbose=False),
                chain1=TransportChain([tr0], verbose=False))


@pytest.fixture(scope="module")
def surface3():
    """D = 3: the surface map (sources cut to 100) and the Matern 3/2 dynamics of examples/dynamics_rollout_3d.py on the demonstration."""
    from gaussian_process_transportation_amd import TransportChain
    g = load_golden("surface_3d")
    tr0 = _fit_transport(dict(g, source=g["source"][:100], target=g["target"][:100]))
    X = g["demo"]
    delta = np.zeros_like(X)
    delta[:-1] = X[1:] - X[:-1]
    dyn = _fit_gp(X, delta, np.sqrt(0.1), [1.0, 1.0, 1.0], 0.01, 1.5, matern_derivatives=True)
    chain = TransportChain([tr0], verbose=False)
    Xs = np.ascontiguousarray(X[::len(X) // M9][:M9] + 0.01)
    return dict(chain=chain, dyn=dyn, X=Xs, y0=np.ascontiguousarray(chain.transport(Xs)[0]), nu=1.5)


def _fold_starts(letter2):
    """test_policy_rollout.test_end_rule's starts: with max_passes = 1 the first four end at step 0 (their guesses are 3 units
    off), the rest go on for at least a step."""
    chain, g = letter2["chain1"], letter2["g"]
    demo = np.ascontiguousarray(g["demo"])
    moved = np.ascontiguousarray(chain.transport(demo)[0])
    _, at = chain.inverse_transport(moved, x0=demo, return_info=True, rtol=RTOL)
    fold, rest = np.flatnonzero(at["stage_det"][0] <= 0), np.flatnonzero(at["stage_det"][0] > 0)
    idx = np.concatenate([fold[:6], rest[:: len(rest) // 3][:3]])
    y0, x0 = moved[idx], demo[idx].copy()
    x0[:4] += 3.0
    return np.ascontiguousarray(y0), np.ascontiguousarray(x0), dict(rtol=1e-2, max_passes=1)


# ------------------------------------------------------------------------------------------------------------ 1. gain = 0
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["K=0 2-D", "K=1 2-D", "K=2 2-D", "K=0 3-D", "K=1 3-D", "K=1 ends"])
def test_gain_zero_is_the_mean_rollout(which, letter2, surface3):
    """path, vel, x, steps_done and status of gain = 0 are those of the merged rollout, NaN positions included."""
    solver = dict(rtol=RTOL)
    if which.endswith("3-D"):
        chain, dyn = (None if which.startswith("K=0") else surface3["chain"]), surface3["dyn"]
        y0, X = (surface3["X"], None) if chain is None else (surface3["y0"], surface3["X"])
    elif which == "K=1 ends":
        chain, dyn = letter2["chain1"], letter2["gp_dyn"]
        y0, X, solver = _fold_starts(letter2)
    else:
        chain = {"K=0": None, "K=1": letter2["chain1"], "K=2": letter2["chain"]}[which[:3]]
        dyn = letter2["gp_dyn"]
        y0, X = _letter_starts(letter2["g"])
        if chain is None:
            y0, X = X, None
    if chain is None:
        solver = {}
    for x0 in ((None,) if chain is None else (None, X)):
        for dt in (0.5, -1.0, 0.3):
            got, want = _stab(chain, dyn, y0, T12, 0.0, dt=dt, x0=x0, **solver), _mean(chain, dyn, y0, T12, dt=dt, x0=x0, **solver)
            print(f"{which} x0={'yes' if x0 is not None else 'no'} dt={dt}: steps done {list(want['steps_done'])}, status {list(want['status'])}")
            _same(got, want, f"{which} x0={x0 is not None} dt={dt}", MEAN_NAMES)
            _check_nan_layout(got)
    if which == "K=1 ends":
        assert np.all(got["steps_done"][:4] == 0) and np.all(got["status"][:4] == INV.MAX_PASSES) and np.any(np.isnan(got["path"]))


# ------------------------------------------------------------------------------------------------------------ 2. and 3.
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["K=0 2-D", "K=1 2-D", "K=2 2-D", "K=0 3-D", "K=1 3-D"])
def test_variance_velocity_and_step(which, letter2, surface3):
    if which.endswith("3-D"):
        chain, dyn, nu = (None if which.startswith("K=0") else surface3["chain"]), surface3["dyn"], 1.5
        y0, X = (surface3["X"], None) if chain is None else (surface3["y0"], surface3["X"])
        gain, dt = 1.0, 1.0
    else:
        chain = {"K=0": None, "K=1": letter2["chain1"], "K=2": letter2["chain"]}[which[:3]]
        dyn, nu = letter2["gp_dyn"], None
        y0, X = _letter_starts(letter2["g"])
        if chain is None:
            y0, X = X, None
        gain, dt = 2.0, 0.5
    solver = {} if chain is None else dict(rtol=RTOL)
    out = _stab(chain, dyn, y0, T12, gain, dt=dt, x0=X, **solver)
    assert out["path"].shape == (M9, T12 + 1, y0.shape[1]) and out["var"].shape == (M9, T12) and out["dvar"].shape == (M9, T12, y0.shape[1])
    assert np.any(out["steps_done"] > 0)
    _check_nan_layout(out)
    _check_variance(out, dyn, nu, which)
    _check_velocity(out, gain, dt, np.sqrt(dyn._noise), which, chain=chain, dyn=dyn, x0_first=X, **solver)
    # the stabiliser does something: the path differs from the mean rollout's, and f is the mean at x
    assert not np.array_equal(out["path"], _mean(chain, dyn, y0, T12, dt=dt, x0=X, **solver)["path"])
    rec = _recorded(out)
    xq = np.ascontiguousarray(np.stack([out["x"][m, t] for m, t in rec]))
    f = np.stack([out["f"][m, t] for m, t in rec])
    assert np.all(np.abs(f - dyn.predict(xq).reshape(f.shape)) <= 1e-9 * np.max(np.abs(f)))


@pytest.mark.gpu
def test_one_step_is_the_minimum_variance_field(surface3):
    """n_steps = 1 from a grid of starts with gain 2: vel is the field of the reference's plot_vector_field_minvar, formed here from
    predict(return_std=True) and derivative_of_variance of the same model."""
    dyn = surface3["dyn"]
    lo, hi = dyn.X.min(axis=0), dyn.X.max(axis=0)
    grid = np.ascontiguousarray(np.stack(np.meshgrid(*[np.linspace(a, b, 3) for a, b in zip(lo, hi)]), axis=-1).reshape(-1, 3))
    path, info = dyn.rollout(grid, 1, return_info=True, variance_gain=2.0)
    mean, std = dyn.predict(grid, return_std=True)
    grad = dyn.derivative_of_variance(grid).T
    want = mean - 2.0 * std.reshape(len(grid), -1)[:, :1] * grad / np.linalg.norm(grad, axis=1)[:, None]
    assert np.all(np.abs(info["vel"][:, 0] - want) <= 1e-9 * np.max(np.abs(want)))
    assert_array_equal(path[:, 1], grid + info["vel"][:, 0])


# ------------------------------------------------------------------------------------------------------------ 4. independence
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
from tests.test_policy_rollout import _letter_starts
from tests.test_rollout_stabilised import _stab, ALL_NAMES
from tests.test_pullback_chain import _fit_rings
from tests.test_pullback_policy import _fit_gp, _fit_transport, RTOL
from tests.conftest import load_golden
from gaussian_process_transportation_amd import TransportChain
g = load_golden("letterS_2d")
chain = TransportChain([_fit_transport(g), _fit_rings(g["traj"][200])], verbose=False)
dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01)
y0, X = _letter_starts(g)
out = _stab(chain, dyn, y0, 12, 1.5, dt=0.5, x0=X, rtol=RTOL)
np.savez(sys.argv[1], **{{k: out[k] for k in ALL_NAMES}})
"""


@pytest.mark.gpu
def test_independence(letter2, tmp_path, monkeypatch):
    """A trajectory's values do not depend on M, on the others, on their order, on which wave of a workgroup owns it or on where
    the launches are cut: every output, bit for bit."""
    chain, dyn = letter2["chain"], letter2["gp_dyn"]
    y0, X = _letter_starts(letter2["g"])
    run = lambda y, x, **kw: _stab(chain, dyn, np.ascontiguousarray(y), T12, 1.5, dt=0.5, x0=np.ascontiguousarray(x), rtol=RTOL, **kw)
    base = run(y0, X)
    assert np.any(base["steps_done"] == T12)
    for m in range(M9):                                          # alone, against inside M = 9
        alone = run(y0[m:m + 1], X[m:m + 1])
        for k in ALL_NAMES:
            assert_array_equal(alone[k][0], base[k][m], err_msg=f"{k}, trajectory {m} alone")
    perm = np.random.default_rng(3).permutation(M9)              # the starts permuted: other neighbours, other waves
    shuffled = run(y0[perm], X[perm])
    for k in ALL_NAMES:
        assert_array_equal(shuffled[k], base[k][perm], err_msg=f"{k} permuted")
    for M in (1, 3, 4, 5):                                       # a workgroup partly filled, exactly filled, one more
        few = run(y0[:M], X[:M])
        for k in ALL_NAMES:
            assert_array_equal(few[k], base[k][:M], err_msg=f"{k} M = {M}")
    # the launch cuts: in this process (read per call) ...
    for per in ("1", "5"):
        monkeypatch.setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", per)
        _same(run(y0, X), base, f"{per} steps per launch, this process")
    monkeypatch.delenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")
    # ... and set before a fresh process starts: 1, 5 and the default
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    for per in ("1", "5", None):
        result = tmp_path / f"child_{per}.npz"
        env = {k: v for k, v in os.environ.items() if k != "GPT_ROLLOUT_STEPS_PER_LAUNCH"}
        if per is not None:
            env["GPT_ROLLOUT_STEPS_PER_LAUNCH"] = per
        subprocess.run([sys.executable, str(script), str(result)], check=True, timeout=300, env=env)
        child = np.load(result)
        _same({k: child[k] for k in ALL_NAMES}, base, f"{per or 'default'} steps per launch, a fresh process")


@pytest.mark.gpu
def test_workgroup_with_early_ends(letter2):
    """One workgroup in which one, and one in which three, of the four trajectories end at step 0 (the letter-S fold with
    max_passes = 1): the survivors equal themselves run alone, and the ended ones their own runs."""
    chain, dyn = letter2["chain1"], letter2["gp_dyn"]
    y0, x0, solver = _fold_starts(letter2)
    bad, good = [0, 1, 2, 3], [4, 5, 6, 7]
    order = np.array([bad[0], good[0], good[1], good[2], bad[1], bad[2], bad[3], good[3]])
    run = lambda idx: _stab(chain, dyn, np.ascontiguousarray(y0[idx]), T12, 1.0, dt=0.5, x0=np.ascontiguousarray(x0[idx]), **solver)
    both = run(order)
    print(f"early ends: steps done {list(both['steps_done'])}, status {list(both['status'])}")
    assert np.all(both["steps_done"][[0, 4, 5, 6]] == 0) and np.all(both["status"][[0, 4, 5, 6]] == INV.MAX_PASSES)
    assert np.all(both["steps_done"][[1, 2, 3, 7]] >= 1)
    _check_nan_layout(both)
    for pos, i in enumerate(order):
        alone = run(np.array([i]))
        for k in ALL_NAMES:
            assert_array_equal(both[k][pos], alone[k][0], err_msg=f"{k}, start {i} at place {pos}")
    _check_velocity(both, 1.0, 0.5, np.sqrt(dyn._noise), "early ends", chain=chain, dyn=dyn, x0_first=np.ascontiguousarray(x0[order]), **solver)


# ------------------------------------------------------------------------------------------------------------ 5. sweep edges
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 65, 511, 512, 513, 1024])
def test_sweep_edges(N):
    """Synthetic dynamics at the sizes where the sweep changes shape: a row tile, a row group, a 512-tile of the packed factor
    and two (1024 crosses into the off-diagonal tile); D = 1, 2, 3 and the three kernels with derivatives; M = 5, T = 3, K = 0."""
    for D in (1, 2, 3):
        for nu in (None, 1.5, 2.5):
            rng = np.random.default_rng(1000 * N + 10 * D + int(2 * (nu or 0)))
            X = rng.uniform(0, 1, (N, D))
            ls = np.array([0.2, 0.3, 0.25])[:D] * (1.0 if D > 1 else 0.25)
            gp = _fit_gp(X, 0.1 * (np.cos(3 * X) - 0.5), 0.5, ls, 1e-3, nu, matern_derivatives=nu is not None)
            y0 = np.ascontiguousarray(rng.uniform(0.1, 0.9, (5, D)))
            out = _stab(None, gp, y0, 3, 1.0, dt=0.05)
            what = f"N = {N}, D = {D}, {KIND[nu]}"
            assert np.all(out["steps_done"] == 3) and np.all(out["status"] == INV.CONVERGED), what
            _check_variance(out, gp, nu, what)
            _check_velocity(out, 1.0, 0.05, np.sqrt(gp._noise), what)


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def _raw(stages, hd, M, T, y0, x0, outs, gain=1.0, std_offset=0.1, K=None, dt=0.5, rtol=RTOL, max_passes=64, entry="gpt_rollout_stabilised"):
    """The C entry point itself on numpy arrays, as tests/test_policy_rollout.py::_raw.  Returns (rc, message)."""
    from gaussian_process_transportation_amd import _lib
    C = _lib.C
    addr = lambda a: None if a is None else a.ctypes.data
    arr = None
    if stages is not None:
        arr = (_lib.ChainStage * max(1, len(stages)))()
        for k, (h, R, c_src, c_dst, scale, R_jac) in enumerate(stages):
            arr[k] = _lib.ChainStage(None if h is None else h._h, addr(R), addr(c_src), addr(c_dst), addr(R_jac), float(scale))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
    ptr = lambda k: ip(outs.get(k)) if k in _lib.ROLLOUT_INT_OUTPUTS else _lib.dptr(outs.get(k))
    y_, x0_ = _lib.dptr(y0), _lib.dptr(x0)
    if entry.endswith("_dev"):                     # (every refusal asked of the device entry comes before it looks at an array)
        ptr, y_, x0_ = (lambda k: None), None, None
    rc = getattr(_lib.load(), entry)(arr, (len(stages) if stages is not None else 0) if K is None else K, None if hd is None else hd._h, y_, x0_, M, T,
                                     float(dt), float(rtol), int(max_passes), float(gain), float(std_offset),
                                     *(ptr(k) for k in _lib.ROLLOUT_STAB_OUTPUTS))
    return rc, _lib.last_error()


def _stab_sentinels(M, T, D):
    from tests.test_pullback_policy import SENT
    return dict(_sentinels(M, T, D), f=np.full((M, T, D), SENT), var=np.full((M, T), SENT), dvar=np.full((M, T, D), SENT))


@pytest.mark.gpu
def test_refusals_and_models_untouched(letter2):
    from gaussian_process_transportation_amd import _lib
    case = letter2
    hd, stages = case["gp_dyn"]._handle, _stage_tuples(case)
    chain, gp_dyn = case["chain"], case["gp_dyn"]
    y = np.ascontiguousarray(case["g"]["traj"][:4])
    probes = [m._handle for m in case["maps"]] + [hd]
    before = [h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd) for h in probes]
    _stab(chain, gp_dyn, y, 3, 1.0)
    _mean(chain, gp_dyn, y, 3)                                   # variance_gain=None: today's path
    outs = _stab_sentinels(4, 3, 2)

    def refused(match, st=stages, hhd=hd, M=4, T=3, drop=(), code=_lib.GPT_E_ARG, dev=True, **kw):
        for entry in ("gpt_rollout_stabilised",) + (("gpt_rollout_stabilised_dev",) if dev else ()):
            rc, msg = _raw(st, hhd, M, T, y, None, {k: v for k, v in outs.items() if k not in drop}, entry=entry, **kw)
            assert rc == code and match in msg, (entry, match, rc, msg)
        assert all(_untouched(v) for v in outs.values()), match

    rng = np.random.default_rng(0)
    X2 = rng.uniform(0, 1, (30, 2))
    # the dynamics: more than 1024 training points
    big = rng.uniform(0, 1, (1025, 2))
    large = _fit_gp(big, 0.05 * np.sin(big), 0.1, [0.3], 1e-2)
    refused("1025 training points", hhd=large._handle)
    refused("at most 1024", st=None, K=0, hhd=large._handle)
    # a dynamics without derivatives
    m12 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, 0.3, 1e-3, 0.5, matern_derivatives=True)
    refused("Matern 1/2 (nu = 0.5) dynamics", hhd=m12._handle)
    refused("Matern 1/2 (nu = 0.5) dynamics", st=None, K=0, hhd=m12._handle)
    for nu in (1.5, 2.5):
        plain = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, 0.3, 1e-3, nu)
        refused("gpt_set_matern_derivatives(h_dyn, 1)", hhd=plain._handle)
        refused("gpt_set_matern_derivatives(h_dyn, 1)", st=None, K=0, hhd=plain._handle)
    # multi-task and fp32 models, as the mean rollout refuses them
    f32 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, [0.3], 1e-3, dtype="float32")
    refused("fp64 models only (the dynamics", hhd=f32._handle)
    multi = _lib.Handle(0)
    Z = rng.uniform(0, 1, (12, 2))
    A_ = rng.standard_normal((2, 12, 12))
    Sigma = np.ascontiguousarray(A_ @ A_.transpose(0, 2, 1) / 12 + 0.1 * np.eye(12))
    multi.fit_svgp(Z, rng.standard_normal((2, 12)), Sigma, np.array([0.3, 0.3]), np.array([1.0, 0.8]), 1e-2)
    refused("single-task models only (the dynamics", hhd=multi)
    # the gain and the offset
    for bad in (-1e-3, -1.0, float("nan"), float("inf"), -float("inf")):
        refused("gain must be finite and >= 0", gain=bad)
    refused("std_offset must be finite", std_offset=float("nan"))
    # the mean rollout's own, in the same words
    refused("K must be 0 .. 4", K=5)
    refused("NULL handle (dynamics)", hhd=None)
    refused("n_steps must be >= 0", T=-1)
    refused("dt must be finite and not zero", dt=0.0)
    refused("rtol", rtol=0.0)
    refused("below 2^31", M=2 ** 15, T=2 ** 16 - 1)
    for name in ("path", "steps_done", "status"):
        refused("must not be NULL", drop=(name,), dev=False)
    # the Python front ends refuse the same before any device call
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="variance_gain must be finite and >= 0"):
            chain.rollout(gp_dyn, y, 3, variance_gain=bad)
        with pytest.raises(ValueError, match="variance_gain must be finite and >= 0"):
            gp_dyn.rollout(y, 3, variance_gain=bad)
    with pytest.raises(ValueError, match="1025 training points"):
        large.rollout(y, 3, variance_gain=1.0)
    with pytest.raises(ValueError, match="1025 training points"):
        chain.rollout(large, y, 3, variance_gain=1.0)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        m12.rollout(X2[:3], 2, variance_gain=1.0)
    with pytest.raises(NotImplementedError, match="matern_derivatives=True"):
        plain.rollout(X2[:3], 2, variance_gain=1.0)
    assert np.all(np.isfinite(large.rollout(y, 2, dt=0.1)))      # without the gain the large model rolls out as before
    assert np.all(np.isfinite(m12.rollout(X2[:3], 2, dt=0.1)))
    # optional outputs: what was not asked for is not written, the rest does not change
    base = _stab(chain, gp_dyn, y, 3, 1.0, dt=0.5, rtol=RTOL)
    for asked in ((), ("var",), ("vel", "dvar"), ("x", "f", "var")):
        o = _stab_sentinels(6, 3, 2)
        rc, msg = _raw(stages, hd, 4, 3, y, None, {k: v for k, v in o.items() if k in asked or k in ("path", "steps_done", "status")},
                       std_offset=np.sqrt(gp_dyn._noise))
        assert rc == _lib.GPT_OK, msg
        for k in ALL_NAMES:
            if k in asked or k in ("path", "steps_done", "status"):
                assert_array_equal(o[k][:4], base[k], err_msg=f"{k} with {asked}")
                assert _untouched(o[k][4:]), k
            else:
                assert _untouched(o[k]), k
    rc, _ = _raw(stages, hd, 0, 3, y, None, outs)                # M = 0 does nothing
    assert rc == _lib.GPT_OK and all(_untouched(v) for v in outs.values())
    none = _stab(chain, gp_dyn, y, 0, 1.0)                       # T = 0: the starts
    assert none["path"].shape == (4, 1, 2) and none["var"].shape == (4, 0) and np.all(none["steps_done"] == 0)
    assert_array_equal(none["path"][:, 0], y)
    multi.close()
    # every model predicts exactly what it did before the rollouts
    for h, was in zip(probes, before):
        now = h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd)
        for k in was:
            if was[k] is not None:
                assert_array_equal(now[k], was[k], err_msg=k)
