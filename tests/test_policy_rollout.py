"""Whole paths of the transported policy in one device call: gpt_rollout_policy (csrc/gpt_rollout.hip: the per-point body of
k_chain_velocity in a loop over the steps, one wave per trajectory), TransportChain.rollout, PolicyTransportation.rollout_policy,
GaussianProcess.rollout.

The call is DEFINED to equal the host loop over the existing call: per step TransportChain.transported_policy(dynamics, y_t,
x0=x_{t-1}, return_info=True) and y_{t+1} = y_t + dt * vel in numpy, a trajectory ending at the first step that is not CONVERGED or
whose next point is not finite (tests/rollout_restatement.rollout, the loop; the device call is its `step`).  So the checks are
bit for bit, NaN positions included (assert_array_equal), and need no tolerance — but one: without maps (K = 0) there is no
existing wave-level call to loop over, and a step's mean is held against predict() at the same point by the floor both carry,
64 eps S each (tests/pullback_restatement.exact_at: "f"), as tests/test_pullback_policy.py::test_python_level holds f against predict.

Models as tests/test_pullback_chain.py builds them: the letter-S golden map (20 points), the rings (36), the dynamics on the
demonstration (400).  M = 9 (the last workgroup is partly filled), T = 12 unless said otherwise."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import inverse_map_restatement as INV
from tests import pullback_restatement as P
from tests import rollout_restatement as RO
from tests.conftest import load_golden
from tests.test_pullback_chain import _case, _fit_rings, _synthetic_stage, rings
from tests.test_pullback_policy import EPS, ISENT, LD, RTOL, SENT, _fit_gp, _fit_transport, _model_of, _synthetic_case, _untouched, sk_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M9, T12 = 9, 12
F_FLOOR = 64 * EPS            # pullback_restatement.exact_at: a wave-strided mean is within 64 eps S of its exact value
NAMES = ("path", "vel", "x", "steps_done", "status")


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.fixture(scope="module")
def oracle_chain():
    """The two-stage fixture of tests/test_pullback_chain.py on the oracle: letter-S, the rings, the dynamics on the demonstration."""
    from oracle.gp_oracle import GaussianProcessOracle
    from tests.test_pullback_chain import _oracle_stage
    g = load_golden("letterS_2d")
    s0 = _oracle_stage(g["source"], g["target"], g["constant_value"], g["length_scale"], g["noise_level"])
    s1 = _oracle_stage(*rings(g["traj"][200]), 4.0, [6.0, 6.0], 1e-3)
    dyn = GaussianProcessOracle(0.3, [1.5, 2.5], 0.01).fit(g["demo"], g["delta"])
    X = np.ascontiguousarray(g["demo"][::45][:M9])
    return {"g": g, "models": [s0["model"], s1["model"]], "affs": [s0["aff"], s1["aff"]], "dyn_model": P.oracle_model(dyn), "X": X,
            "y": s1["fwd"](s0["fwd"](X))}


def test_restated_step_is_the_chain_restatement(oracle_chain):
    """Step t of the restated rollout is tests/chain_restatement.chain at y_t with x0 = x_{t-1}, and y_{t+1} = y_t + dt * vel_t."""
    from tests import chain_restatement as CH
    c = oracle_chain
    for x0, dt in ((None, 1.0), (c["X"], 0.5), (c["X"], -1.0)):
        out = RO.rollout(RO.chain_step(c["models"], c["dyn_model"], c["affs"], rtol=RTOL), c["y"], 3, dt=dt, x0=x0)
        assert out["path"].shape == (M9, 4, 2) and out["vel"].shape == (M9, 3, 2) and out["x"].shape == (M9, 3, 2)
        assert_array_equal(out["path"][:, 0], c["y"])
        guess = x0
        for t in range(3):
            live = out["steps_done"] >= t
            assert np.any(live)
            y = np.ascontiguousarray(out["path"][live, t])
            one = CH.chain(c["models"], c["dyn_model"], c["affs"], y, x0=None if guess is None else np.ascontiguousarray(guess[live]), rtol=RTOL)
            assert_array_equal(out["x"][live, t], one["x"])
            assert_array_equal(out["vel"][live, t], one["vel"])
            went = out["steps_done"] > t
            assert_array_equal(out["path"][went, t + 1], out["path"][went, t] + dt * out["vel"][went, t])
            guess = out["x"][:, t]
        assert np.all(out["steps_done"][out["status"] == INV.CONVERGED] == 3)           # (nothing here leaves the finite numbers)
    back = RO.rollout(RO.chain_step(c["models"], c["dyn_model"], c["affs"], rtol=RTOL), c["y"], 2, dt=-1.0, x0=c["X"])
    fwd = RO.rollout(RO.chain_step(c["models"], c["dyn_model"], c["affs"], rtol=RTOL), c["y"], 2, dt=1.0, x0=c["X"])
    assert_array_equal(back["vel"][:, 0], fwd["vel"][:, 0])                               # a negative dt: the same policy, the other way
    assert_array_equal(back["path"][:, 1], c["y"] - fwd["vel"][:, 0])
    assert_array_equal(fwd["path"][:, 1], c["y"] + fwd["vel"][:, 0])


def test_restated_end_rule():
    """A trajectory that ends at step 0, in the middle (by its status, and by leaving the finite numbers) and never; T = 0."""
    T = 5
    y0 = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [10.0, 10.0]])
    seen = []

    def step(y, guess):
        # trajectory 0 (y < 0.5) never converges; 1 stalls once it has passed 3; 2 overflows at its third step; 3 goes on
        seen.append((y.copy(), None if guess is None else guess.copy()))
        status = np.where(y[:, 0] < 0.5, INV.MAX_PASSES, np.where((y[:, 0] >= 3.0) & (y[:, 0] < 3.5), INV.STALLED, INV.CONVERGED))
        vel = np.where((y[:, :1] >= 4.0) & (y[:, :1] < 4.5), 1e308, 1.0) * np.ones_like(y)
        return y - 10.0, vel, status.astype(np.int32)

    out = RO.rollout(step, y0, T, dt=2.0, x0=y0 + 7.0)
    # 0: ends at step 0.  1: 1 -> 3 (stalled at step 1).  2: 2 -> 4 -> (4 + 2e308 = inf: ends at step 1, CONVERGED).  3: never
    assert list(out["steps_done"]) == [0, 1, 1, T]
    assert list(out["status"]) == [INV.MAX_PASSES, INV.STALLED, INV.CONVERGED, INV.CONVERGED]
    for m, done in enumerate(out["steps_done"]):
        assert np.all(np.isfinite(out["path"][m, :done + 1])) and np.all(np.isnan(out["path"][m, done + 1:]))
        last = min(done + 1, T)                              # the step that ended the trajectory is still recorded
        assert np.all(np.isfinite(out["vel"][m, :last])) and np.all(np.isnan(out["vel"][m, last:]))
        assert np.all(np.isfinite(out["x"][m, :last])) and np.all(np.isnan(out["x"][m, last:]))
    assert_array_equal(out["path"][3, :, 0], 10.0 + 2.0 * np.arange(T + 1))
    assert_array_equal(out["x"][0, 0], y0[0] - 10.0)
    # the guesses: x0 at step 0, then the x of the step before, of the trajectories still alive, in their order
    assert_array_equal(seen[0][1], y0 + 7.0)
    assert_array_equal(seen[1][0], out["path"][1:, 1])
    assert_array_equal(seen[1][1], out["x"][1:, 0])
    assert len(seen[2][0]) == 1 and len(seen) == T
    # T = 0: the starts, nothing evaluated
    none = RO.rollout(step, y0, 0, dt=1.0)
    assert none["path"].shape == (4, 1, 2) and none["vel"].shape == (4, 0, 2) and len(seen) == T
    assert_array_equal(none["path"][:, 0], y0)
    assert list(none["steps_done"]) == [0] * 4 and list(none["status"]) == [INV.CONVERGED] * 4
    # without x0 the first step gets no guess
    RO.rollout(step, y0[3:], 1)
    assert seen[-1][1] is None


def test_restated_rollout_without_maps(oracle_chain):
    c = oracle_chain
    out = RO.rollout(RO.mean_step(c["dyn_model"]), c["X"], 4, dt=0.5)
    assert np.all(out["steps_done"] == 4) and np.all(out["status"] == INV.CONVERGED)
    assert_array_equal(out["x"], out["path"][:, :-1])
    for t in range(4):
        assert_array_equal(out["vel"][:, t], c["dyn_model"].mean(out["path"][:, t])[0].astype(np.float64))
        assert_array_equal(out["path"][:, t + 1], out["path"][:, t] + 0.5 * out["vel"][:, t])


def test_python_refusals_need_no_device():
    from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportation, TransportChain
    from gaussian_process_transportation_amd.policy_transportation import PolicyTransportation
    g = load_golden("letterS_2d")
    y = g["traj"][:3]
    new = lambda **kw: GaussianProcess(kernel=sk_kernel(0.1, [0.3], 1e-3), optimizer=None, verbose=False, **kw)

    class NoRollout:
        def fit(self, X, Y): pass
        def pullback_policy(self, *a, **k): pass
        def pullback_chain(self, *a, **k): pass

    def fitted(method):
        pt = PolicyTransportation(method, verbose=False)
        pt.fit(g["source"], g["target"])
        return pt

    # an unfitted model rolling out itself, and as the dynamics or a map of a chain
    with pytest.raises(RuntimeError, match="not fitted"):
        new().rollout(y, 5)
    with pytest.raises(RuntimeError, match="not fitted"):
        new().rollout_chain([], new(), y, 5, [None])
    with pytest.raises(ValueError, match="1 .. 4 maps, got 5"):
        new().rollout_chain([new() for _ in range(4)], new(), y, 5, [None] * 5)
    with pytest.raises(ValueError, match="2 maps, 1 affine"):
        new().rollout_chain([new()], new(), y, 5, [None])
    # wrong kinds: a dynamics that is no GaussianProcess, a delta_map without rollout_chain
    with pytest.raises(NotImplementedError, match="dynamics .NoRollout. must be a fitted GaussianProcess"):
        new().rollout_chain([], NoRollout(), y, 5, [None])
    with pytest.raises(NotImplementedError, match="map of stage 0 .NoRollout."):
        new().rollout_chain([NoRollout()], new(), y, 5, [None] * 2)
    chain = TransportChain([fitted(NoRollout())], verbose=False)
    with pytest.raises(NotImplementedError, match="NoRollout.*rollout_chain"):
        chain.rollout(new(), y, 5)
    with pytest.raises(TypeError, match="tolerance"):
        chain.rollout(new(), y, 5, tolerance=1.0)
    with pytest.raises(NotImplementedError, match="NoRollout"):
        fitted(NoRollout()).rollout_policy(new(), y, 5)
    tr = GaussianProcessTransportation(optimizer=None, verbose=False)
    tr.method = fitted(NoRollout())
    with pytest.raises(NotImplementedError, match="NoRollout"):
        tr.rollout_policy(new(), y, 5)


# ------------------------------------------------------------------------------------------------------------ GPU
def _host_loop(chain, dyn, y0, T, dt=1.0, x0=None, **solver):
    """The loop the device call replaces: one transported_policy call per step, y + dt * vel in numpy."""
    def step(y, guess):
        vel, info = chain.transported_policy(dyn, y, x0=guess, return_info=True, **solver)
        return info["x"], vel, info["status"]
    return RO.rollout(step, y0, T, dt=dt, x0=x0)


def _device(chain, dyn, y0, T, dt=1.0, x0=None, **solver):
    path, info = chain.rollout(dyn, y0, T, dt=dt, x0=x0, return_info=True, **solver)
    return dict(info, path=path)


def _same(got, want, what):
    for k in NAMES:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def _letter_starts(g, traj="traj"):
    """(starts on the moved demonstration, their source-space preimages): M = 9."""
    idx = np.arange(M9) * 44
    return np.ascontiguousarray(g[traj][idx]), np.ascontiguousarray(g["demo"][idx])


@pytest.fixture(scope="module")
def letter2():
    from gaussian_process_transportation_amd import TransportChain
    g = load_golden("letterS_2d")
    tr0, tr1 = _fit_transport(g), _fit_rings(g["traj"][200])
    dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01)
    return dict(_case([tr0, tr1], dyn, [None, None]), g=g, chain=TransportChain([tr0, tr1], verbose=False),
                chain1=TransportChain([tr0], verbose=False))


@pytest.fixture(scope="module")
def letter3():
    """A do_scale=True first stage, the rings, a Matern 5/2 stage with its analytic derivatives, and a Matern 1/2 dynamics."""
    from gaussian_process_transportation_amd import TransportChain
    g = load_golden("letterS_2d")
    trs = [_fit_transport(g, do_scale=True), _fit_rings(g["traj2"][200]), _fit_rings(g["traj2"][100], nu=2.5, push=(1.0, 0.25, 0.0))]
    dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01, 0.5)
    return dict(_case(trs, dyn, [None, None, 2.5], 0.5), g=g, chain=TransportChain(trs, verbose=False))


def _four_stages_3d():
    """K = GPT_CHAIN_MAX at D = 3, as tests/test_pullback_chain.py::test_four_stages_3d."""
    from gaussian_process_transportation_amd import TransportChain
    g = load_golden("surface_3d")
    tr0 = _fit_transport(dict(g, source=g["source"][:100], target=g["target"][:100]))
    rng = np.random.default_rng(11)
    moved = tr0.method.transport(g["demo"], return_std=False)[0]
    lo, hi = moved.min(axis=0), moved.max(axis=0)
    trs = [tr0] + [_synthetic_stage(rng.uniform(lo, hi, (40 + 13 * k, 3)), k, 0.4) for k in range(1, 4)]
    dyn = _fit_gp(g["demo"], g["delta"], 0.05, [0.5, 0.6, 0.7], 1e-4, 1.5)
    chain = TransportChain(trs, verbose=False)
    X = np.ascontiguousarray(g["demo"][::len(g["demo"]) // M9][:M9])
    return chain, dyn, np.ascontiguousarray(chain.transport(X)[0]), X


def _one_stage_1d():
    """K = 1 at D = 1: the synthetic case of tests/test_pullback_policy.py behind the attributes TransportChain reads."""
    from gaussian_process_transportation_amd import TransportChain
    c = _synthetic_case(1, 64, 100, None, 1.5)
    a = c["aff"]
    method = types.SimpleNamespace(delta_map=c["gp_map"], verbose=False, affine_transform=types.SimpleNamespace(
        rotation_matrix=a["R"], scale=a["scale"], S_centroid=a["c_src"], T_centroid=a["c_dst"]))
    X = a["c_src"] + np.linspace(-0.3, 0.3, M9)[:, None]
    gam = P.affine_forward(a, X)
    y = np.ascontiguousarray(gam + c["gp_map"].predict(gam).reshape(M9, 1))
    return TransportChain([method], verbose=False), c["gp_dyn"], y, np.ascontiguousarray(X)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["K=1", "K=2", "K=3", "K=4 3-D", "K=1 1-D"])
def test_definition_bit_for_bit(which, letter2, letter3):
    """path, vel, x, steps_done and status equal the host loop over transported_policy, with and without x0, dt = 1, 0.5, -1 and 0.3."""
    if which == "K=4 3-D":
        chain, dyn, y0, X = _four_stages_3d()
    elif which == "K=1 1-D":
        chain, dyn, y0, X = _one_stage_1d()
    else:
        case = letter3 if which == "K=3" else letter2
        chain, dyn = case["chain1" if which == "K=1" else "chain"], case["gp_dyn"]
        y0, X = _letter_starts(case["g"], "traj2" if which == "K=3" else "traj")
    for x0 in (None, X):
        for dt in (1.0, 0.5, -1.0, 0.3):           # (0.3: dt * vel is not exact, a fused multiply-add across the step would show)
            got, want = _device(chain, dyn, y0, T12, dt=dt, x0=x0, rtol=RTOL), _host_loop(chain, dyn, y0, T12, dt=dt, x0=x0, rtol=RTOL)
            print(f"{which} x0={'yes' if x0 is not None else 'no'} dt={dt}: steps done {list(want['steps_done'])}, status {list(want['status'])}")
            _same(got, want, f"{which} x0={x0 is not None} dt={dt}")
            assert got["path"].shape == (M9, T12 + 1, y0.shape[1]) and np.any(want["steps_done"] > 0)


@pytest.mark.gpu
def test_one_step_no_step_no_trajectory(letter2):
    chain, dyn = letter2["chain"], letter2["gp_dyn"]
    y0, X = _letter_starts(letter2["g"])
    one = _device(chain, dyn, y0, 1, dt=0.5, x0=X, rtol=RTOL)
    vel, info = chain.transported_policy(dyn, y0, x0=X, return_info=True, rtol=RTOL)
    assert_array_equal(one["vel"][:, 0], vel)
    assert_array_equal(one["x"][:, 0], info["x"])
    assert_array_equal(one["status"], info["status"])
    assert np.all(info["status"] == INV.CONVERGED) and np.all(one["steps_done"] == 1)
    assert_array_equal(one["path"][:, 1], y0 + 0.5 * vel)
    none = _device(chain, dyn, y0, 0, x0=X)
    assert none["path"].shape == (M9, 1, 2) and none["vel"].shape == (M9, 0, 2) and none["x"].shape == (M9, 0, 2)
    assert_array_equal(none["path"][:, 0], y0)
    assert np.all(none["steps_done"] == 0) and np.all(none["status"] == INV.CONVERGED)
    assert_array_equal(chain.rollout(dyn, y0, 0), none["path"])                     # (without return_info: the path alone)
    empty = _device(chain, dyn, np.zeros((0, 2)), T12)
    assert empty["path"].shape == (0, T12 + 1, 2) and empty["vel"].shape == (0, T12, 2) and empty["steps_done"].shape == (0,)
    # the K = 1 front ends are the one-stage chain
    tr0 = letter2["tr"][0]
    a = tr0.rollout_policy(dyn, y0, 3, dt=0.5, x0=X, rtol=RTOL)
    b, info_b = tr0.method.rollout_policy(dyn, y0, 3, dt=0.5, x0=X, return_info=True, rtol=RTOL)
    assert_array_equal(a, _device(letter2["chain1"], dyn, y0, 3, dt=0.5, x0=X, rtol=RTOL)["path"])
    assert_array_equal(a, b)
    assert set(info_b) == {"vel", "x", "steps_done", "status"}


@pytest.mark.gpu
def test_end_rule(letter2):
    """max_passes = 1 where the letter-S map folds: a step converges only where its guess already solves it.  Starts on the moved
    demonstration with their preimages as guesses do; the same starts with guesses 3 units off do not and end at step 0; the
    others end once the path has left the guess (max_passes = 1 never moves it) by more than the tolerance, or never."""
    chain, dyn, g = letter2["chain1"], letter2["gp_dyn"], letter2["g"]
    demo = np.ascontiguousarray(g["demo"])
    moved = np.ascontiguousarray(chain.transport(demo)[0])
    _, at = chain.inverse_transport(moved, x0=demo, return_info=True, rtol=RTOL)
    fold = np.flatnonzero(at["stage_det"][0] <= 0)                          # where the map folds: det(I + J_psi) is not positive there
    print(f"end rule: the map folds at {len(fold)} of {len(moved)} demonstration points")
    assert len(fold) >= 6
    rest = np.flatnonzero(at["stage_det"][0] > 0)
    idx = np.concatenate([fold[:6], rest[:: len(rest) // 3][:3]])
    y0, x0 = moved[idx], demo[idx].copy()
    x0[:4] += 3.0
    solver = dict(rtol=1e-2, max_passes=1)
    _, first = chain.inverse_transport(y0, x0=x0, return_info=True, **solver)
    assert np.all(first["status"][:4] != INV.CONVERGED) and np.all(first["status"][4:] == INV.CONVERGED)
    got = _device(chain, dyn, y0, T12, dt=0.5, x0=x0, **solver)
    want = _host_loop(chain, dyn, y0, T12, dt=0.5, x0=x0, **solver)
    print(f"end rule: steps done {list(want['steps_done'])}, status {list(want['status'])}")
    _same(got, want, "max_passes=1")
    assert np.all(got["steps_done"][:4] == 0) and np.all(got["status"][:4] == INV.MAX_PASSES)
    assert np.all(got["steps_done"][4:] >= 1)
    for m, done in enumerate(got["steps_done"]):
        assert np.all(np.isfinite(got["path"][m, :done + 1])) and np.all(np.isnan(got["path"][m, done + 1:]))
        last = min(done + 1, T12)                            # the step that ended the trajectory is still recorded
        for k in ("vel", "x"):
            assert np.all(np.isfinite(got[k][m, :last])) and np.all(np.isnan(got[k][m, last:])), (k, m)
        assert (got["status"][m] == INV.CONVERGED) == (done == T12)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
from tests.test_policy_rollout import _letter_starts, _device, NAMES
from tests.test_pullback_chain import _fit_rings
from tests.test_pullback_policy import _fit_gp, _fit_transport, RTOL
from tests.conftest import load_golden
from gaussian_process_transportation_amd import TransportChain
g = load_golden("letterS_2d")
chain = TransportChain([_fit_transport(g), _fit_rings(g["traj"][200])], verbose=False)
dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01)
y0, X = _letter_starts(g)
out = _device(chain, dyn, y0, 12, dt=0.5, x0=X, rtol=RTOL)
np.savez(sys.argv[1], **{{k: out[k] for k in NAMES}})
"""


@pytest.mark.gpu
def test_independence(letter2, tmp_path, monkeypatch):
    """A trajectory's values do not depend on M, on the others, on their order or on where the launches are cut."""
    chain, dyn = letter2["chain"], letter2["gp_dyn"]
    y0, X = _letter_starts(letter2["g"])
    base = _device(chain, dyn, y0, T12, dt=0.5, x0=X, rtol=RTOL)
    rev = _device(chain, dyn, np.ascontiguousarray(y0[::-1]), T12, dt=0.5, x0=np.ascontiguousarray(X[::-1]), rtol=RTOL)
    for k in NAMES:
        assert_array_equal(rev[k][::-1], base[k], err_msg=k)
    for m in (0, 4):
        alone = _device(chain, dyn, y0[m:m + 1], T12, dt=0.5, x0=X[m:m + 1], rtol=RTOL)
        for k in NAMES:
            assert_array_equal(alone[k][0], base[k][m], err_msg=k)
    at = np.arange(M9) * 7 + 3                                   # embedded in M = 70, among other trajectories
    filler, filler_x = np.ascontiguousarray(letter2["g"]["traj"][5:75]), np.ascontiguousarray(letter2["g"]["demo"][5:75])
    filler[at], filler_x[at] = y0, X
    many = _device(chain, dyn, filler, T12, dt=0.5, x0=filler_x, rtol=RTOL)
    for k in NAMES:
        assert_array_equal(many[k][at], base[k], err_msg=k)
    # 5 steps per launch (three launches, the last x carried between them) against the default (one launch): read per call ...
    monkeypatch.setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", "5")
    _same(_device(chain, dyn, y0, T12, dt=0.5, x0=X, rtol=RTOL), base, "5 steps per launch, this process")
    monkeypatch.delenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")
    # ... and set before a fresh process starts
    script, result = tmp_path / "child.py", tmp_path / "child.npz"
    script.write_text(_CHILD.format(root=ROOT))
    subprocess.run([sys.executable, str(script), str(result)], check=True, timeout=300, env=dict(os.environ, GPT_ROLLOUT_STEPS_PER_LAUNCH="5"))
    child = np.load(result)
    _same({k: child[k] for k in NAMES}, base, "5 steps per launch, a fresh process")


@pytest.mark.gpu
def test_host_chunk_boundary(letter2):
    """T = 255: chunks of 131072 / 256 = 512 trajectories.  M = 513 with the 20-point map alone walks both staging sets."""
    chain, dyn, g = letter2["chain1"], letter2["gp_dyn"], letter2["g"]
    T, M = 255, 513
    y0 = np.ascontiguousarray(np.tile(g["traj"], (2, 1))[:M] + np.linspace(0.0, 0.5, M)[:, None])
    whole = _device(chain, dyn, y0, T, dt=0.1, rtol=RTOL)
    first, last = _device(chain, dyn, y0[:512], T, dt=0.1, rtol=RTOL), _device(chain, dyn, y0[512:], T, dt=0.1, rtol=RTOL)
    for k in NAMES:
        assert_array_equal(whole[k][:512], first[k], err_msg=k)
        assert_array_equal(whole[k][512:], last[k], err_msg=k)
    assert whole["path"].shape == (M, T + 1, 2)
    print(f"chunk boundary: {int(np.sum(whole['steps_done'] == T))} of {M} trajectories complete")


def _raw(stages, hd, M, T, y0, x0, outs, K=None, dt=0.5, rtol=RTOL, max_passes=64, entry="gpt_rollout_policy"):
    """The C entry point itself on numpy arrays.  stages: [(handle or None, R, c_src, c_dst, scale, R_jac)] or None; outs: name ->
    array or None.  Returns (rc, message)."""
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
                                     float(dt), float(rtol), int(max_passes), *(ptr(k) for k in _lib.ROLLOUT_OUTPUTS))
    return rc, _lib.last_error()


def _stage_tuples(case, K=None):
    return [(m._handle, a["R"], a["c_src"], a["c_dst"], a["scale"], a.get("R_jac", a["R"])) for m, a in zip(case["maps"][:K], case["affs"][:K])]


def _sentinels(M, T, D):
    return {"path": np.full((M, T + 1, D), SENT), "vel": np.full((M, T, D), SENT), "x": np.full((M, T, D), SENT),
            "steps_done": np.full(M, ISENT, dtype=np.int32), "status": np.full(M, ISENT, dtype=np.int32)}


@pytest.mark.gpu
def test_optional_outputs(letter2):
    """vel and x NULL in every combination, x0 present or not: the other outputs do not change, what was not asked for is not written."""
    from gaussian_process_transportation_amd import _lib
    chain, dyn = letter2["chain"], letter2["gp_dyn"]
    hd, stages = dyn._handle, _stage_tuples(letter2)
    y0, X = _letter_starts(letter2["g"])
    for x0 in (None, X):
        base = _device(chain, dyn, y0, T12, dt=0.5, x0=x0, rtol=RTOL)
        for asked in ((), ("vel",), ("x",), ("vel", "x")):
            outs = _sentinels(M9 + 2, T12, 2)                    # two rows more than M: they stay sentinels
            rc, msg = _raw(stages, hd, M9, T12, y0, x0, {k: v for k, v in outs.items() if k in asked or k not in ("vel", "x")})
            assert rc == _lib.GPT_OK, msg
            for k in NAMES:
                if k in asked or k not in ("vel", "x"):
                    assert_array_equal(outs[k][:M9], base[k], err_msg=f"{k} with {asked}")
                    assert _untouched(outs[k][M9:]), k
                else:
                    assert _untouched(outs[k]), k
    few = chain.rollout(dyn, y0, T12, dt=0.5, rtol=RTOL)
    assert_array_equal(few, _device(chain, dyn, y0, T12, dt=0.5, rtol=RTOL)["path"])


@pytest.mark.gpu
def test_device_entry(letter2):
    """gpt_rollout_policy_dev on torch tensors equals the host entry."""
    import torch
    case, dyn = letter2, letter2["gp_dyn"]
    y0, X = _letter_starts(letter2["g"])
    base = _device(letter2["chain"], dyn, y0, T12, dt=0.5, x0=X, rtol=RTOL)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    keep = [[t(a["R"]), t(a["c_src"]), t(a["c_dst"])] for a in case["affs"]]
    dstages = [(m._handle, R.data_ptr(), cs.data_ptr(), cd.data_ptr(), a["scale"], R.data_ptr()) for m, a, (R, cs, cd) in zip(case["maps"], case["affs"], keep)]
    yd, xd = t(y0), t(X)
    h_last = case["maps"][-1]._handle
    for asked in (("vel", "x"), ()):
        outs = {k: torch.from_numpy(v).to(dev) for k, v in _sentinels(M9, T12, 2).items()}
        h_last.rollout_policy_dev(dstages, dyn._handle, yd.data_ptr(), M9, T12, outs["path"].data_ptr(), outs["steps_done"].data_ptr(),
                                  outs["status"].data_ptr(), dt=0.5, x0_ptr=xd.data_ptr(), rtol=RTOL,
                                  **{k + "_ptr": outs[k].data_ptr() for k in asked})
        h_last.synchronize()
        for k in NAMES:
            if k in asked or k not in ("vel", "x"):
                assert_array_equal(outs[k].cpu().numpy(), base[k], err_msg=k)
            else:
                assert _untouched(outs[k].cpu().numpy()), k


@pytest.mark.gpu
def test_model_rolls_out_itself():
    """K = 0 on the Matern 5/2 dynamics: every recorded step is path[t] + dt * f_t exactly, f_t the mean at path[t]."""
    g = load_golden("letterS_2d")
    dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01, 2.5)
    model = _model_of(dyn, 2.5)
    y0 = np.ascontiguousarray(g["demo"][np.arange(M9) * 44])
    for dt in (1.0, -0.5):
        path, info = dyn.rollout(y0, T12, dt=dt, return_info=True)
        assert path.shape == (M9, T12 + 1, 2) and np.all(info["steps_done"] == T12) and np.all(info["status"] == INV.CONVERGED)
        assert_array_equal(path[:, 0], y0)
        assert_array_equal(info["x"], path[:, :-1])
        share = 0.0
        for t in range(T12):
            assert_array_equal(path[:, t + 1], path[:, t] + dt * info["vel"][:, t])
            at = np.ascontiguousarray(path[:, t])
            exact, S = model.mean(at)
            ref = dyn.predict(at)
            tol = F_FLOOR * S
            assert np.all(np.abs(info["vel"][:, t].astype(LD) - exact) <= tol)
            assert np.all(np.abs(info["vel"][:, t].astype(LD) - ref.astype(LD)) <= 2 * tol)
            share = max(share, float(np.max(np.abs(info["vel"][:, t].astype(LD) - ref.astype(LD)) / (2 * tol))))
        print(f"K = 0, dt = {dt}: f_t against predict(path[t]), largest share of 2 x 64 eps S {share:.3f}")
        assert_array_equal(dyn.rollout(y0, T12, dt=dt), path)
    # independent of the launch cut and of M here too
    one = dyn.rollout(y0[3:4], T12, dt=1.0)
    assert_array_equal(one[0], dyn.rollout(y0, T12, dt=1.0)[3])


@pytest.mark.gpu
def test_refusals_and_models_untouched(letter2):
    from gaussian_process_transportation_amd import _lib
    case = letter2
    hd, stages = case["gp_dyn"]._handle, _stage_tuples(case)
    y = np.ascontiguousarray(case["g"]["traj"][:4])
    probes = [m._handle for m in case["maps"]] + [hd]
    before = [h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd) for h in probes]
    _device(case["chain"], case["gp_dyn"], y, 3)
    outs = _sentinels(4, 3, 2)

    def refused(match, st=stages, hhd=hd, M=4, T=3, y_=y, x0_=None, drop=(), code=_lib.GPT_E_ARG, dev=True, **kw):
        for entry in ("gpt_rollout_policy",) + (("gpt_rollout_policy_dev",) if dev else ()):
            rc, msg = _raw(st, hhd, M, T, y_, x0_, {k: v for k, v in outs.items() if k not in drop}, entry=entry, **kw)
            assert rc == code and match in msg, (entry, match, rc, msg)
        assert all(_untouched(v) for v in outs.values()), match

    swap = lambda k, **f: [tuple(f.get(n, v) for n, v in zip(("h", "R", "c_src", "c_dst", "scale", "R_jac"), s)) if i == k else s for i, s in enumerate(stages)]
    # gpt_pullback_chain's refusals, with K = 0 allowed
    refused("K must be 0 .. 4", K=-1)
    refused("K must be 0 .. 4", K=5)
    refused("stages must not be NULL", st=None, K=2)
    refused("NULL handle (stage 0 map)", st=swap(0, h=None))
    refused("NULL handle (dynamics)", hhd=None)
    refused("NULL handle (dynamics)", st=None, K=0, hhd=None)
    empty = _lib.Handle(0)
    refused("stage 1 map model is not fitted", st=swap(1, h=empty), code=_lib.GPT_E_STATE)
    refused("dynamics model is not fitted", hhd=empty, code=_lib.GPT_E_STATE)
    refused("dynamics model is not fitted", st=None, K=0, hhd=empty, code=_lib.GPT_E_STATE)
    refused("stages 0 and 1 are the same handle", st=swap(1, h=stages[0][0]))
    refused("stage 1 and h_dyn are the same handle", hhd=stages[1][0])
    for name in ("R", "c_src", "c_dst", "R_jac"):
        refused("must not be NULL (stage 1)", st=swap(1, **{name: None}))
    rng = np.random.default_rng(0)
    X2, X3 = rng.uniform(0, 1, (30, 2)), rng.uniform(0, 1, (30, 3))
    three_d = _fit_gp(X3, 0.05 * np.sin(X3), 0.1, [0.3], 1e-3)
    refused("share one space", st=swap(0, h=three_d._handle))
    refused("share one space", hhd=three_d._handle)
    two_out = _fit_gp(X3, X3[:, :2], 0.1, [0.3], 1e-3)
    refused("the stage 0 map model must map a space onto itself", st=swap(0, h=two_out._handle))
    refused("the dynamics model must map a space onto itself", st=None, K=0, hhd=two_out._handle)          # K = 0: the dynamics alone
    f32 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, [0.3], 1e-3, dtype="float32")
    refused("fp64 models only (the stage 1 map", st=swap(1, h=f32._handle))
    refused("fp64 models only (the dynamics", hhd=f32._handle)
    refused("fp64 models only (the dynamics", st=None, K=0, hhd=f32._handle)
    m12 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, 0.3, 1e-3, 0.5, matern_derivatives=True)
    refused("Matern 1/2", st=swap(0, h=m12._handle))
    m52 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, 0.3, 1e-3, 2.5)
    refused("gpt_set_matern_derivatives", st=swap(1, h=m52._handle))
    for bad in (0.0, -1e-3, float("nan")):
        refused("rtol", rtol=bad)
    refused("max_passes", max_passes=0)
    # the rollout's own
    refused("n_steps must be >= 0", T=-1)
    for bad in (0.0, float("nan"), float("inf"), -float("inf")):
        refused("dt must be finite and not zero", dt=bad)
    refused("2^31", M=-1)
    refused("2^31", M=2 ** 31, T=0)
    refused("below 2^31", M=2 ** 15, T=2 ** 16 - 1)
    refused("below 2^31", M=1, T=2 ** 31 - 1)
    refused("must not be NULL", y_=None, dev=False)
    for name in ("path", "steps_done", "status"):
        refused("must not be NULL", drop=(name,), dev=False)
    nan_at = lambda a, i: np.ascontiguousarray(np.where(np.arange(a.size).reshape(a.shape) == i, np.nan, a))
    refused("NaN or infinity", y_=nan_at(y, 3), dev=False)
    refused("NaN or infinity", x0_=nan_at(y, 0), dev=False)
    refused("NaN or infinity", st=swap(0, scale=float("inf")), dev=False)
    refused("NaN or infinity", st=swap(1, c_dst=np.full(2, np.nan)), dev=False)
    # the Python front ends refuse the same before any device call
    chain, gp_dyn = case["chain"], case["gp_dyn"]
    for bad in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dt must be finite and not zero"):
            chain.rollout(gp_dyn, y, 3, dt=bad)
        with pytest.raises(ValueError, match="dt must be finite and not zero"):
            gp_dyn.rollout(y, 3, dt=bad)
    with pytest.raises(ValueError, match="n_steps must be an integer >= 0"):
        chain.rollout(gp_dyn, y, -1)
    with pytest.raises(ValueError, match="n_steps must be an integer >= 0"):
        chain.rollout(gp_dyn, y, 2.5)
    with pytest.raises(ValueError, match="below 2\\^31"):
        chain.rollout(gp_dyn, y, 2 ** 30)
    with pytest.raises(ValueError, match="x0 has shape"):
        chain.rollout(gp_dyn, y, 3, x0=y[:2])
    with pytest.raises(ValueError, match="starts has 3 columns"):
        chain.rollout(gp_dyn, np.zeros((2, 3)), 3)
    with pytest.raises(NotImplementedError, match="float64 models only"):
        chain.rollout(f32, y, 3)
    with pytest.raises(NotImplementedError, match="float64 models only"):
        f32.rollout(y, 3)
    with pytest.raises(NotImplementedError, match="space onto itself"):
        two_out.rollout(X3[:2], 3)
    with pytest.raises(ValueError, match="one object twice"):
        chain.rollout(case["maps"][0], y, 3)
    aff = [(a["R"], a["scale"], a["c_src"], a["c_dst"], None) for a in case["affs"]]
    with pytest.raises(NotImplementedError, match="matern_derivatives=True"):           # a Matern map without its derivatives
        case["maps"][1].rollout_chain([m52], gp_dyn, y, 3, aff)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        case["maps"][1].rollout_chain([m12], gp_dyn, y, 3, aff)
    with pytest.raises(ValueError, match="the last map has 2 features, the dynamics 3"):
        chain.rollout(three_d, y, 3)
    # M = 0 does nothing; a Matern 1/2 model is fine as the dynamics and on its own
    rc, _ = _raw(stages, hd, 0, 3, y, None, outs)
    assert rc == _lib.GPT_OK and all(_untouched(v) for v in outs.values())
    assert np.all(np.isfinite(m12.rollout(X2[:3], 2, dt=0.1)))
    empty.close()
    # every model predicts exactly what it did before the rollouts
    for h, was in zip(probes, before):
        now = h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd)
        for k in was:
            if was[k] is not None:
                assert was[k].tobytes() == now[k].tobytes(), k
