"""Whole paths of whole functions drawn from the dynamics posterior in one device call: gpt_rollout_pathwise
(csrc/gpt_rollout_pathwise.hip: k_rollout's step with ch_mean on the function's own weights and the sum over the random Fourier
features), _lib.Handle.rollout_pathwise, GaussianProcess.sample_functions / rollout_chain_functions, PosteriorFunctions,
TransportChain.rollout_functions and the transport classes' rollout_policy_functions.

What holds the kernel:
  1. anchor: J = 0 with weights = alpha is the mean rollout, bit for bit (every line of the body but the feature sum's own); zero
     draws with J = 130 through the public interface are rollout() but for the sign of a zero.
  2. independence of M S, the other paths and functions, their order, the launch cuts and the host chunks, bit for bit.
  3. values: one step's f against the longdouble restatement (tests/pathwise_restatement.function_values) within
     32 max(e_oracle, 2^-53 sum of the absolute terms, a feature term weighted by 1 + |theta_j|), e_oracle the fp64 restatement
     against the longdouble one; through maps, x is pullback_chain's bit for bit and vel is f pushed through its stage_A, within the
     4 ulps tests/test_rollout_stabilised.py holds the push of a vector to.
  4. ends.  5. refusals.  6. the device entry, a path whose func names no function; functions belong to their fit.
Models as tests/test_policy_rollout.py: the letter-S map (20 points), the rings (36), the dynamics on the demonstration (400)."""
import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import pathwise_restatement as PW
from tests.test_policy_rollout import M9, T12, _letter_starts, _stage_tuples
from tests.test_pullback_policy import EPS, LD, RTOL, _fit_gp
from tests.test_rollout_stabilised import _fold_starts, _mean, _pushed, letter2, surface3      # noqa: F401 (fixtures)

MEAN_NAMES = ("path", "vel", "x", "steps_done", "status")
ALL_NAMES = ("path", "vel", "x", "f", "steps_done", "status")
NU = {"rbf": None, "matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


# ------------------------------------------------------------------------------------------------------------ helpers
def _pw(case, K, dyn, y0, func, weights, omega, amp, T, dt=1.0, x0=None, rtol=RTOL, max_passes=64):
    """The device call on the handles: the first K stages of `case` (K = 0: the dynamics rolls out itself)."""
    stages = _stage_tuples(case, K) if K else []
    owner = stages[-1][0] if K else dyn._handle
    return owner.rollout_pathwise(stages, dyn._handle, np.ascontiguousarray(y0), func, weights, omega, amp, T, dt=dt,
                                  x0=None if x0 is None else np.ascontiguousarray(x0), rtol=rtol, max_passes=max_passes)


def _mean_functions(dyn, S=1):
    """weights = alpha for every function, no frequency."""
    D = dyn.X.shape[1]
    return np.repeat(dyn.gp.alpha_[None], S, axis=0), np.zeros((0, D)), np.zeros((S, 0, 2, D))


def _drawn(dyn, S, J, seed=0, scale=1.0):
    """weights (S,N,D), omega (J,D) = scale x a draw of the product's own, amp (S,J,2,D): functions drawn from the posterior of `dyn`
    (a Matern 1/2 model, which sample_functions refuses: its alpha, perturbed; the kernel does not ask where the numbers come from)."""
    rs = np.random.RandomState(seed)
    N, D = dyn.X.shape
    ls = np.broadcast_to(np.asarray(dyn._ls, dtype=np.float64), (D,))
    omega = np.ascontiguousarray(scale * rs.standard_normal((J, D)) / ls)
    if dyn._ktype != 1:
        fn = dyn.sample_functions(n_functions=S, frequencies=omega, random_state=seed)
        return fn.weights, fn.omega, fn.amplitudes
    weights = dyn.gp.alpha_[None] + 0.01 * np.abs(dyn.gp.alpha_).max() * rs.standard_normal((S, N, D))
    amp = np.sqrt(dyn._c / max(J, 1)) * rs.standard_normal((S, J, 2, D))
    return np.ascontiguousarray(weights), omega, np.ascontiguousarray(amp)


def _same(got, want, what, names=ALL_NAMES):
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def _small_dyn(N, D, nu=None, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.uniform(-1.5, 1.5, (N, D))
    Y = 0.2 * np.cos(X @ rs.standard_normal((D, D))) - 0.1 * X
    return _fit_gp(X, Y, 0.5, [0.8] * D, 0.01, nu)


# ------------------------------------------------------------------------------------------------------------ 1. anchor
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["K=0 2-D", "K=1 2-D", "K=2 2-D", "K=0 3-D", "K=1 3-D", "K=1 ends"])
def test_no_features_and_alpha_is_the_mean_rollout(which, letter2, surface3):
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
    fn = dyn.sample_functions(frequencies=np.zeros((0, y0.shape[1])), draws=(np.zeros((2, 0, 2, y0.shape[1])), np.zeros((2,) + dyn.X.shape)))
    assert_array_equal(fn.weights, np.repeat(dyn.gp.alpha_[None], 2, axis=0))      # zero draws: V = alpha, bit for bit
    for x0 in ((None,) if chain is None else (None, X)):
        for dt in (0.5, -1.0):
            want = _mean(chain, dyn, y0, T12, dt=dt, x0=x0, **solver)
            if chain is None:
                path, info = fn.rollout(y0, T12, dt=dt, return_info=True)
            else:
                path, info = chain.rollout_functions(fn, y0, T12, dt=dt, x0=x0, return_info=True, **solver)
            got = dict(info, path=path)
            print(f"{which} x0={'yes' if x0 is not None else 'no'} dt={dt}: steps done {list(want['steps_done'])}, status {list(want['status'])}")
            for j in range(2):
                _same({k: v[:, j] for k, v in got.items()}, want, f"{which} x0={x0 is not None} dt={dt} function {j}", MEAN_NAMES)
            # f is the drawn function at x: here the mean, which vel is for K = 0
            if chain is None:
                assert_array_equal(got["f"], got["vel"])
    if which == "K=1 ends":
        assert np.all(got["steps_done"][:4] == 0) and np.any(np.isnan(got["path"])) and np.all(np.isnan(got["f"][:4, :, 1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("D,N", [(1, 5), (1, 65), (2, 5), (2, 64), (2, 65), (2, 130), (3, 65)])
def test_anchor_at_the_edges_of_the_source_loop(D, N):
    """K = 0, N below, at and past the 64 lanes of a wave and past two rounds of them, in every dimension."""
    dyn = _small_dyn(N, D, seed=N)
    y0 = np.ascontiguousarray(dyn.X[:: max(1, N // 5)][:5] + 0.05)
    want = _mean(None, dyn, y0, T12, dt=0.5)
    w, om, amp = _mean_functions(dyn)
    got = _pw(None, 0, dyn, y0, np.zeros(len(y0), dtype=np.int32), w, om, amp, T12, dt=0.5)
    _same(got, want, f"D={D} N={N}", MEAN_NAMES)
    assert np.all(got["steps_done"] == T12)


@pytest.mark.gpu
def test_zero_draws_with_frequencies_are_the_mean_rollout(letter2):
    """J = 130 with zero amplitudes: the feature sum runs and adds a zero."""
    dyn = letter2["gp_dyn"]
    _, X = _letter_starts(letter2["g"])
    om = np.random.RandomState(0).standard_normal((130, 2))
    fn = dyn.sample_functions(frequencies=om, draws=(np.zeros((3, 130, 2, 2)), np.zeros((3,) + dyn.X.shape)))
    want, info = dyn.rollout(X, T12, return_info=True)
    got, ginfo = fn.rollout(X, T12, return_info=True)
    assert got.shape == (M9, 3, T12 + 1, 2)
    for j in range(3):
        assert_array_equal(got[:, j], want)
        assert_array_equal(ginfo["vel"][:, j], info["vel"])
        assert_array_equal(ginfo["steps_done"][:, j], info["steps_done"])
    mean = dyn.predict(X)
    assert_array_equal(fn.predict(X), np.repeat(ginfo["f"][None, :, 0, 0], 3, axis=0))
    assert np.all(np.abs(fn.predict(X) - mean[None]) <= 1e-12 * np.abs(mean).max())


# ------------------------------------------------------------------------------------------------------------ 2. independence
@pytest.mark.gpu
def test_a_path_does_not_depend_on_its_surroundings(letter2, monkeypatch):
    dyn, T = letter2["gp_dyn"], 7
    y3, x3 = (a[:3] for a in _letter_starts(letter2["g"]))
    w, om, amp = _drawn(dyn, 3, 65, seed=1)
    y0, x0 = np.repeat(y3, 3, axis=0), np.repeat(x3, 3, axis=0)      # path = start * 3 + function
    func = np.tile(np.arange(3, dtype=np.int32), 3)
    run = lambda idx, **kw: _pw(letter2, 2, dyn, y0[idx], func[idx], w, om, amp, T, dt=0.5, x0=x0[idx], **kw)
    every = np.arange(9)
    among = run(every)
    print(f"independence: steps done {list(among['steps_done'])}, status {list(among['status'])}")
    assert np.sum(among["steps_done"] == T) >= 6 and not np.array_equal(among["path"][0], among["path"][1])
    for n in (1, 4, 5):                                          # M S = 1, 4, 5 against 9: a lone wave, a full workgroup, one past it
        _same(run(every[:n]), {k: v[:n] for k, v in among.items()}, f"the first {n} paths")
    perm = np.random.RandomState(3).permutation(9)
    _same(run(perm), {k: v[perm] for k, v in among.items()}, "shuffled")
    for s in range(3):                                           # S = 1 against S = 3
        idx = every[func == s]
        alone = _pw(letter2, 2, dyn, y0[idx], np.zeros(3, dtype=np.int32), w[s:s + 1], om, amp[s:s + 1], T, dt=0.5, x0=x0[idx])
        _same(alone, {k: v[idx] for k, v in among.items()}, f"function {s} alone")
    for per in ("1", "3"):                                       # launches cut after every step and inside the path
        monkeypatch.setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", per)
        _same(run(every), among, f"{per} steps per launch")
    monkeypatch.delenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")
    monkeypatch.setenv("GPT_ROLLOUT_PATHWISE_CHUNK", "4")        # host chunks of 4, 4 and 1 paths
    _same(run(every), among, "three host chunks")
    monkeypatch.setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", "3")
    _same(run(every), among, "three host chunks, 3 steps per launch")
    monkeypatch.delenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")
    monkeypatch.delenv("GPT_ROLLOUT_PATHWISE_CHUNK")
    # one T-step call against T one-step calls, each from the recorded point with the x of the step before as its guess (the
    # paths that reached step t)
    for t in range(T):
        at = np.flatnonzero(among["steps_done"] >= t)
        one = _pw(letter2, 2, dyn, among["path"][at, t], func[at], w, om, amp, 1, dt=0.5, x0=x0[at] if t == 0 else among["x"][at, t - 1])
        for k in ("vel", "x", "f"):
            assert_array_equal(one[k][:, 0], among[k][at, t], err_msg=f"step {t} on its own: {k}")
        assert_array_equal(one["path"][:, 1], among["path"][at, t + 1], err_msg=f"step {t} on its own: path")
        assert_array_equal(one["steps_done"], (among["steps_done"][at] > t).astype(np.int32))


# ------------------------------------------------------------------------------------------------------------ 3. values
_RATIOS = []


def _check_values(what, dyn, kind, weights, omega, amp, func, x, f):
    ref, floor = PW.function_values(dyn.X, dyn._c, dyn._ls, kind, weights, omega, amp, func, x)
    ref64, _ = PW.function_values(dyn.X, dyn._c, dyn._ls, kind, weights, omega, amp, func, x, ty=np.float64)
    e_oracle = np.abs(ref64.astype(LD) - ref).astype(np.float64)
    err = np.abs(f.astype(LD) - ref).astype(np.float64)
    bound = np.maximum(e_oracle, 2.0 ** -53 * floor.astype(np.float64))
    ratio = float(np.max(err / bound))
    theta = float(np.max(np.abs(x @ omega.T))) if omega.shape[0] else 0.0
    print(f"ratio {what} J={omega.shape[0]} largest |theta| {theta:.3g}: {ratio:.2f}   (gpu {float(err.max()):.2e}, oracle {float(e_oracle.max()):.2e}, "
          f"floor {float(2.0 ** -53 * floor.max()):.2e})")
    _RATIOS.append(ratio)
    assert ratio <= 32, what


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rbf", "matern12", "matern32", "matern52"])
def test_one_step_values(kind):
    """K = 0, x = y exactly: f of one step against the longdouble restatement, J below, at and past the lanes of a wave."""
    dyn = _small_dyn(130, 2, NU[kind], seed=4)
    x = np.ascontiguousarray(np.random.RandomState(5).uniform(-1.5, 1.5, (9, 2)))
    func = (np.arange(9) % 3).astype(np.int32)
    for J in (1, 63, 64, 65, 130):
        w, om, amp = _drawn(dyn, 3, J, seed=J)
        out = _pw(None, 0, dyn, x, func, w, om, amp, 1)
        assert_array_equal(out["x"][:, 0], x)
        assert_array_equal(out["vel"], out["f"])
        _check_values(f"{kind}", dyn, kind, w, om, amp, func, x, out["f"][:, 0])
    # frequencies large enough that theta is about 1e5: the argument reduction of the sine and cosine
    w, om, amp = _drawn(dyn, 3, 65, seed=9, scale=1e5)
    out = _pw(None, 0, dyn, x, func, w, om, amp, 1)
    assert np.max(np.abs(x @ om.T)) > 5e4
    _check_values(f"{kind} large theta", dyn, kind, w, om, amp, func, x, out["f"][:, 0])
    print(f"largest ratio so far {max(_RATIOS):.2f}")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2])
def test_values_through_maps(K, letter2):
    """x is the chain's own inverse at the same points, bit for bit; f is the function at that x; vel is f pushed through the
    stage_A that pullback_chain returns there."""
    dyn = letter2["gp_dyn"]
    chain = letter2["chain1"] if K == 1 else letter2["chain"]
    y0, X = _letter_starts(letter2["g"])
    w, om, amp = _drawn(dyn, 3, 65, seed=2)
    func = (np.arange(M9) % 3).astype(np.int32)
    out = _pw(letter2, K, dyn, y0, func, w, om, amp, 1, x0=X)
    _, info = chain.transported_policy(dyn, np.ascontiguousarray(y0), x0=np.ascontiguousarray(X), return_info=True, rtol=RTOL)
    assert_array_equal(out["x"][:, 0], info["x"])
    _check_values(f"K={K} rbf", dyn, "rbf", w, om, amp, func, out["x"][:, 0], out["f"][:, 0])
    worst = 0.0
    for m in range(M9):
        want, norm = _pushed(chain, dyn, out, m, 0, out["f"][m, 0], dict(rtol=RTOL, x0_first=X))
        tol = 4 * EPS * np.max(np.abs(out["f"][m, 0])) * norm
        worst = max(worst, float(np.max(np.abs(out["vel"][m, 0] - want))) / tol)
    print(f"K={K}: vel against f pushed through stage_A, largest share of 4 ulps {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ 4. ends
@pytest.mark.gpu
def test_ends(letter2):
    dyn = letter2["gp_dyn"]
    _, X = _letter_starts(letter2["g"])
    w, om, amp = _drawn(dyn, 2, 5, seed=3)
    amp[1] = 1e308                                               # function 1 throws y out of the finite numbers at once
    func = (np.arange(M9) % 2).astype(np.int32)
    out = _pw(None, 0, dyn, X, func, w, om, amp, T12, dt=10.0)
    big = func == 1
    print(f"ends: steps done {list(out['steps_done'])}, status {list(out['status'])}")
    assert np.all(out["steps_done"][big] < T12) and np.any(out["steps_done"][big] == 0) and np.all(out["status"][big] == 0)
    assert_array_equal(out["path"][:, 0], X)
    for m in np.flatnonzero(big):                                # the end rule: the step that ended the path keeps its x, vel and f
        done = int(out["steps_done"][m])
        assert np.all(np.isfinite(out["path"][m, :done + 1])) and np.all(np.isnan(out["path"][m, done + 1:])), m
        assert np.all(np.isfinite(out["x"][m, :done + 1])) and np.all(np.isfinite(out["vel"][m, :done])), m
        for k in ("vel", "x", "f"):
            assert np.all(np.isnan(out[k][m, done + 1:])), (k, m)
    assert np.all(np.isfinite(out["path"][~big, :2]))
    # the others are what they are without the function that overflows
    alone = _pw(None, 0, dyn, X[~big], np.zeros(int((~big).sum()), dtype=np.int32), w[:1], om, amp[:1], T12, dt=10.0)
    _same(alone, {k: v[~big] for k, v in out.items()}, "beside paths that end")
    # negative dt: backwards in time, step by step the same rule
    back = _pw(None, 0, dyn, X, np.zeros(M9, dtype=np.int32), w[:1], om, amp[:1], T12, dt=-0.25)
    assert np.all(back["steps_done"] == T12)
    assert_array_equal(back["path"][:, 1:], back["path"][:, :-1] + (-0.25) * back["vel"])
    # T = 0
    none = _pw(None, 0, dyn, X, func, w, om, amp, 0)
    assert_array_equal(none["path"], X[:, None])
    assert none["vel"].shape == (M9, 0, 2) and none["f"].shape == (M9, 0, 2)
    assert np.all(none["steps_done"] == 0) and np.all(none["status"] == 0)


# ------------------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.gpu
def test_refusals(letter2):
    from gaussian_process_transportation_amd import _lib
    dyn = letter2["gp_dyn"]
    N, D = dyn.X.shape
    _, X = _letter_starts(letter2["g"])
    M, T, S, J = 2, 3, 2, 4
    w, om, amp = _drawn(dyn, S, J)
    y0, func = np.ascontiguousarray(X[:M]), np.zeros(M, dtype=np.int32)
    SENT = -7.25
    out = {"path": np.full((M, T + 1, D), SENT), "vel": np.full((M, T, D), SENT), "x": np.full((M, T, D), SENT), "f": np.full((M, T, D), SENT),
           "steps_done": np.full(M, -77, dtype=np.int32), "status": np.full(M, -77, dtype=np.int32)}
    dp, ip = _lib.dptr, lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))

    def raw(entry="gpt_rollout_pathwise", y0=y0, func=func, M=M, T=T, dt=1.0, S=S, w=w, J=J, om=om, amp=amp, path=out["path"],
            steps=out["steps_done"], status=out["status"]):
        if entry.endswith("_dev"):                               # (refused before any pointer is read)
            rc = getattr(_lib.load(), entry)(None, 0, dyn._handle._h, y0.ctypes.data, None, func.ctypes.data, M, T, dt, 1e-10, 64, S,
                                             None if w is None else w.ctypes.data, J, None if om is None else om.ctypes.data,
                                             None if amp is None else amp.ctypes.data, path.ctypes.data, None, None, None, steps.ctypes.data,
                                             status.ctypes.data)
        else:
            rc = getattr(_lib.load(), entry)(None, 0, dyn._handle._h, dp(y0), None, ip(func), M, T, dt, 1e-10, 64, S, dp(w), J, dp(om), dp(amp), dp(path),
                                             dp(out["vel"]), dp(out["x"]), dp(out["f"]), ip(steps), ip(status))
        return rc, _lib.last_error()

    def refused(match, **kw):
        for entry in ("gpt_rollout_pathwise", "gpt_rollout_pathwise_dev") if kw.pop("both", True) else ("gpt_rollout_pathwise",):
            rc, msg = raw(entry, **kw)
            assert rc == _lib.GPT_E_ARG and match in msg, (entry, kw.keys(), rc, msg)
        assert all(np.all(v == (SENT if v.dtype == np.float64 else -77)) for v in out.values())

    refused("S, the number of functions", S=0)
    refused("S, the number of functions", S=-1)
    refused("J must be 0 .. 8192", J=-1)
    refused("J must be 0 .. 8192", J=_lib.PATHWISE_MAX_FREQ + 1)
    refused("func must not be NULL", func=None, both=False)
    refused("weights must not be NULL", w=None)
    refused("omega and amp must not be NULL", om=None)
    refused("omega and amp must not be NULL", amp=None)
    refused("n_steps must be >= 0", T=-1)
    refused("dt must be finite", dt=0.0)
    refused("y0, path, steps_done and status", path=None, both=False)
    for bad in (np.array([0, S], dtype=np.int32), np.array([-1, 0], dtype=np.int32)):
        refused("is not one of the 2 functions", func=bad, both=False)
    for name, arr in (("w", w), ("om", om), ("amp", amp)):
        for poison in (np.nan, np.inf):
            bad = arr.copy()
            bad.reshape(-1)[-1] = poison
            refused("weights / omega / amp contain NaN or infinity", both=False, **{name: bad})
    rc, msg = raw(y0=np.full((M, D), np.nan))
    assert rc == _lib.GPT_E_ARG and "NaN or infinity" in msg
    assert raw(M=0)[0] == _lib.GPT_OK and np.all(out["path"] == SENT)
    # the Python layer
    h = dyn._handle
    with pytest.raises(ValueError, match="func has shape"):
        h.rollout_pathwise([], h, y0, np.zeros(3, dtype=np.int32), w, om, amp, T)
    with pytest.raises(ValueError, match="func must hold indices"):
        h.rollout_pathwise([], h, y0, np.array([0, 2]), w, om, amp, T)
    with pytest.raises(ValueError, match="weights has shape"):
        h.rollout_pathwise([], h, y0, func, w[:, :-1], om, amp, T)
    with pytest.raises(ValueError, match="omega has shape"):
        h.rollout_pathwise([], h, y0, func, w, om, amp[:, :-1], T)
    with pytest.raises(ValueError, match="at most 8192"):
        h.rollout_pathwise([], h, y0, func, w, np.zeros((8193, D)), np.zeros((S, 8193, 2, D)), T)
    with pytest.raises(TypeError, match="PosteriorFunctions"):
        letter2["chain"].rollout_functions(dyn, y0, T)
    with pytest.raises(TypeError, match="tolerance"):
        letter2["chain"].rollout_functions(dyn.sample_functions(1, 4), y0, T, tolerance=1.0)
    # and the call serves on: the transport classes' entry gives the chain's paths
    fn = dyn.sample_functions(2, 8)
    tr0 = letter2["tr"][0]
    yt = np.ascontiguousarray(letter2["chain1"].transport(X[:M])[0])
    a = tr0.rollout_policy_functions(fn, yt, T, x0=y0)
    b = letter2["chain1"].rollout_functions(fn, yt, T, x0=y0)
    assert a.shape == (M, 2, T + 1, D)
    assert_array_equal(a, b)
    assert_array_equal(a[:, 1:], letter2["chain1"].rollout_functions(fn.subset([1]), yt, T, x0=y0))


# ------------------------------------------------------------------------------------------------------------ 6. the device entry
@pytest.mark.gpu
def test_device_entry_and_a_path_without_a_function(letter2):
    """gpt_rollout_pathwise_dev on torch tensors (the weights as [S][NP][4] images) equals the host entry, launch cuts included; a path
    whose func names no function ends before its first step: steps_done 0, status ROLLOUT_NO_FUNCTION, NaN everywhere, its
    neighbours untouched by it."""
    import torch
    from gaussian_process_transportation_amd import _lib
    dyn, T = letter2["gp_dyn"], 7
    _, X = _letter_starts(letter2["g"])
    w, om, amp = _drawn(dyn, 2, 65, seed=6)
    func = (np.arange(M9) % 2).astype(np.int32)
    base = _pw(None, 0, dyn, X, func, w, om, amp, T, dt=0.5)
    N, D, _, NP = dyn._handle.info()
    img = np.zeros((2, NP, 4))
    img[:, :N, :D] = w
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bad = func.copy()
    bad[[2, 5]] = [2, -1]
    yd, wd, od, ad = t(X), t(img), t(om), t(amp)
    for f_in, per in ((func, None), (bad, "3")):
        fd = t(f_in)
        outs = {"path": np.full((M9, T + 1, D), -7.25), "vel": np.full((M9, T, D), -7.25), "x": np.full((M9, T, D), -7.25), "f": np.full((M9, T, D), -7.25),
                "steps_done": np.full(M9, -77, dtype=np.int32), "status": np.full(M9, -77, dtype=np.int32)}
        outs = {k: t(v) for k, v in outs.items()}
        if per:
            os.environ["GPT_ROLLOUT_STEPS_PER_LAUNCH"] = per
        try:
            dyn._handle.rollout_pathwise_dev([], dyn._handle, yd.data_ptr(), fd.data_ptr(), M9, T, 2, wd.data_ptr(), 65, od.data_ptr(), ad.data_ptr(),
                                             outs["path"].data_ptr(), outs["steps_done"].data_ptr(), outs["status"].data_ptr(), dt=0.5,
                                             vel_ptr=outs["vel"].data_ptr(), x_ptr=outs["x"].data_ptr(), f_ptr=outs["f"].data_ptr())
            dyn._handle.synchronize()
        finally:
            os.environ.pop("GPT_ROLLOUT_STEPS_PER_LAUNCH", None)
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        ok = (f_in >= 0) & (f_in < 2)
        _same({k: v[ok] for k, v in got.items()}, {k: v[ok] for k, v in base.items()}, f"device entry, steps per launch {per}")
        for m in np.flatnonzero(~ok):
            assert got["steps_done"][m] == 0 and got["status"][m] == _lib.ROLLOUT_NO_FUNCTION, m
            assert all(np.all(np.isnan(got[k][m])) for k in ("path", "vel", "x", "f")), m


@pytest.mark.gpu
def test_functions_belong_to_their_fit():
    """Functions drawn before a refit are refused afterwards, also where the new fit has the same sizes."""
    dyn = _small_dyn(20, 2, seed=1)
    fn = dyn.sample_functions(2, 8)
    assert fn.predict(dyn.X[:3]).shape == (2, 3, 2)
    dyn.fit(dyn.X, dyn.Y + 0.5)
    with pytest.raises(RuntimeError, match="fitted again"):
        fn.predict(dyn.X[:3])
    with pytest.raises(RuntimeError, match="fitted again"):
        fn.subset([0]).rollout(dyn.X[:3], 2)
    assert dyn.sample_functions(2, 8).rollout(dyn.X[:3], 2).shape == (3, 2, 3, 2)
