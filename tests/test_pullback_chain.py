"""The transported policy through a chain of transports: gpt_pullback_chain (csrc/gpt_chain.hip: K Newton inverses, affine
inverses, the dynamics mean and the push-forward in one launch; the handles' variance launches; a one-thread-per-query
epilogue), GaussianProcess.pullback_chain, TransportChain.

Fixture (checked on the CPU below).  Stage 0: the letter-S golden map.  Stage 1: three rings of 12 points, radii 3, 9 and 20,
round traj[200], pushed outwards by 2, 0.5 and 0 — an obstacle the moved demonstration bends round — with C(4) RBF([6, 6]) +
White(1e-3).  Dynamics: C(0.3) RBF([1.5, 2.5]) + White(0.01) on demo / delta.  The 20 x 20 grid over the moved trajectory's box
+- 5 converges everywhere at stage 1 and stalls at 3 points at stage 0, so it exercises "a stage that does not converge hands on
the point it reached".

Bounds (no new constants).  The device against the cascade of existing device calls — gpt_pullback_policy per stage from the last
stage to the first, x of one the y of the next — bit for bit for everything the one launch writes per stage, and f.  vel and the
two variances of vel against the chained products in np.longdouble at the arrays the device returned: 16 (K + 1) eps S, S the
same product with absolute values on every term (tests/chain_restatement.py).  var_dyn, stage_Jvar, stage_map_var against
predict_all at the returned x / z_k: VAR_SPLIT_RTOL of the prior variance, as tests/test_pullback_policy.py.  x against a known
preimage: chain_restatement.carried_bound, inverse_map_restatement.error_bound carried through the stages."""
import numpy as np
import pytest

from tests import chain_restatement as CH
from tests import inverse_map_restatement as INV
from tests import pullback_restatement as P
from tests.conftest import load_golden, relmax
from tests.test_pullback_policy import (EPS, G0, HOST_CHUNK, ISENT, LD, RTOL, SENT, VAR_SPLIT_RTOL, _affine_of, _call, _counts, _fit_gp,
                                        _fit_transport, _model_of, _synthetic_case, _untouched, sk_kernel)

STAGE_BITWISE = ("stage_z", "stage_x", "stage_A", "stage_status", "stage_passes", "stage_residual", "stage_det")
ONE_LAUNCH = ("x", "vel", "f", "status") + STAGE_BITWISE


def rings(centre, push=(2.0, 0.5, 0.0), radii=(3.0, 9.0, 20.0), n=12):
    """(source, target): n points on each circle round `centre`, moved outwards by push[i]."""
    ang = 2 * np.pi * np.arange(n) / n
    u = np.column_stack([np.cos(ang), np.sin(ang)])
    return (np.concatenate([centre + r * u for r in radii]), np.concatenate([centre + (r + p) * u for r, p in zip(radii, push)]))


def box_grid(T, n=20, margin=5.0):
    xg, yg = np.meshgrid(np.linspace(T[:, 0].min() - margin, T[:, 0].max() + margin, n),
                         np.linspace(T[:, 1].min() - margin, T[:, 1].max() + margin, n))
    return np.ascontiguousarray(np.column_stack([xg.ravel(), yg.ravel()]))


# ------------------------------------------------------------------------------------------------------------ CPU
def _oracle_stage(src, tgt, c, ls, noise):
    from oracle.gp_oracle import AffineTransformOracle, GaussianProcessOracle
    a = AffineTransformOracle().fit(src, tgt)
    s = a.predict(src)
    gp = GaussianProcessOracle(c, ls, noise).fit(s, tgt - s)
    aff = {"R": np.ascontiguousarray(a.rotation_matrix), "scale": float(getattr(a, "scale", 1.0)), "c_src": a.S_centroid, "c_dst": a.T_centroid}
    return {"a": a, "gp": gp, "aff": aff, "model": P.oracle_model(gp), "fwd": lambda x: a.predict(x) + gp.predict(a.predict(x))}


@pytest.fixture(scope="module")
def oracle_chain():
    from oracle.gp_oracle import GaussianProcessOracle
    g = load_golden("letterS_2d")
    s0 = _oracle_stage(g["source"], g["target"], g["constant_value"], g["length_scale"], g["noise_level"])
    s1 = _oracle_stage(*rings(g["traj"][200]), 4.0, [6.0, 6.0], 1e-3)
    dyn = GaussianProcessOracle(0.3, [1.5, 2.5], 0.01).fit(g["demo"], g["delta"])
    X = g["demo"][::8]
    return {"g": g, "stages": [s0, s1], "models": [s0["model"], s1["model"]], "affs": [s0["aff"], s1["aff"]], "dyn": dyn,
            "dyn_model": P.oracle_model(dyn), "X": X, "y": s1["fwd"](s0["fwd"](X))}


def test_restatement_round_trip(oracle_chain):
    """chain(Phi_1(Phi_0(X)), x0 = X) stays at X, one pass per stage, within the carried inverse bound; vel is the product of the
    oracle's own Jacobians times its own f; without the guess all 50 points converge, in at most 6 and 12 passes."""
    c = oracle_chain
    X, y = c["X"], c["y"]
    out = CH.chain(c["models"], c["dyn_model"], c["affs"], y, x0=X, rtol=RTOL)
    assert np.all(out["status"] == INV.CONVERGED) and np.all(out["stage_passes"] == 1)
    stage_y = [out["stage_x"][1], y]
    bound = CH.carried_bound(c["models"], c["affs"], out["stage_z"], stage_y, RTOL)
    err = np.linalg.norm(out["x"] - X, axis=1)
    print(f"restatement: |x - X| <= {err.max():.2e}, largest share of the carried bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    J = np.broadcast_to(np.eye(2), (len(X), 2, 2))
    pos = X
    for s in c["stages"]:
        gam = s["a"].predict(pos)
        J = ((np.eye(2)[None] + s["gp"].derivative(gam)) @ s["aff"]["R"]) @ J
        pos = gam + s["gp"].predict(gam)
    f = c["dyn"].predict(X)
    assert relmax(out["f"], f) <= 1e-12
    assert relmax(out["vel"], np.einsum("mod,md->mo", J, f)) <= 1e-11
    free = CH.chain(c["models"], c["dyn_model"], c["affs"], y, rtol=RTOL)
    print("restatement without guesses: passes", free["stage_passes"].max(axis=1))
    assert np.all(free["stage_status"] == INV.CONVERGED)
    assert free["stage_passes"][1].max() <= 6 and free["stage_passes"][0].max() <= 12


def test_restatement_single_stage_is_the_pullback(oracle_chain):
    c = oracle_chain
    y = c["g"]["traj"][::8]
    for x0 in (None, c["X"]):
        one = CH.chain(c["models"][:1], c["dyn_model"], c["affs"][:1], y, x0=x0, rtol=RTOL)
        ref = P.pullback(c["models"][0], c["dyn_model"], c["affs"][0], y, x0=x0, rtol=RTOL)
        for k in ("x", "f", "vel", "status"):
            assert one[k].tobytes() == ref[k].tobytes(), k
        for k, r in (("stage_z", "z"), ("stage_A", "A"), ("stage_passes", "passes"), ("stage_residual", "residual"), ("stage_det", "det"),
                     ("stage_x", "x"), ("stage_status", "status")):
            assert one[k][0].tobytes() == ref[r].tobytes(), k


def test_restatement_grid_statuses(oracle_chain):
    c = oracle_chain
    out = CH.chain(c["models"], c["dyn_model"], c["affs"], box_grid(c["g"]["traj"]), rtol=RTOL)
    assert list(_counts(out["stage_status"][1])) == [400, 0, 0, 0]
    assert list(_counts(out["stage_status"][0])) == [397, 0, 0, 3]
    assert np.array_equal(out["status"], CH.first_failing(out["stage_status"])) and list(_counts(out["status"])) == [397, 0, 0, 3]
    assert np.all(np.isfinite(out["vel"]))                          # the stalled points still get a value, at the point reached


def test_restatement_variance_formulas():
    """K = 1 is tests/pullback_restatement.variance_epilogue, every column of vel_var_map its scalar; K = 2 against the formulas
    written out with explicit loops."""
    rng = np.random.default_rng(5)
    M, D = 6, 3
    affs = [{"R": rng.standard_normal((D, D)), "R_jac": rng.standard_normal((D, D))} for _ in range(2)]
    f, A, var_dyn, Jvar = rng.standard_normal((M, D)), np.eye(D) + 0.3 * rng.standard_normal((2, M, D, D)), rng.uniform(0.5, 1, M), rng.uniform(0, 1, (2, M, D))
    one, ref = CH.variances(affs[:1], f, A[:1], var_dyn, Jvar[:1], 0.1), P.variance_epilogue(affs[0], f, A[0], var_dyn, Jvar[0], 0.1)
    assert np.all(np.abs(one["vel_var_dyn"][0] - ref["vel_var_dyn"][0]) <= 4 * np.finfo(LD).eps * np.abs(ref["vel_var_dyn"][0]))
    for i in range(D):
        assert np.all(np.abs(one["vel_var_map"][0][:, i] - ref["vel_var_map"][0]) <= 4 * np.finfo(LD).eps * np.abs(ref["vel_var_map"][0]))
    two = CH.variances(affs, f, A, var_dyn, Jvar, 0.1)
    for m in range(M):
        B0, B1 = A[0, m] @ affs[0]["R_jac"], A[1, m] @ affs[1]["R_jac"]
        s0 = np.sum(Jvar[0, m] * (affs[0]["R_jac"] @ f[m]) ** 2)
        s1 = np.sum(Jvar[1, m] * (affs[1]["R_jac"] @ (B0 @ f[m])) ** 2)
        want_map = s0 * np.sum(B1 ** 2, axis=1) + s1
        want_dyn = (np.sqrt(var_dyn[m]) - 0.1) ** 2 * np.sum((B1 @ B0) ** 2, axis=1)
        assert np.allclose(np.asarray(two["vel_var_map"][0][m], dtype=float), want_map, rtol=1e-12, atol=0)
        assert np.allclose(np.asarray(two["vel_var_dyn"][0][m], dtype=float), want_dyn, rtol=1e-12, atol=0)
    v, tol = CH.velocity(affs, f, A)
    assert np.allclose(np.asarray(v, dtype=float), np.einsum("mij,mjk,mk->mi", A[1] @ affs[1]["R_jac"], A[0] @ affs[0]["R_jac"], f), rtol=1e-12, atol=0)
    assert np.all(tol > 0)


def test_python_refusals_need_no_device():
    from gaussian_process_transportation_amd import GaussianProcess, GaussianProcessTransportation, TransportChain
    from gaussian_process_transportation_amd.policy_transportation import PolicyTransportation
    g, g3 = load_golden("letterS_2d"), load_golden("surface_3d")

    class NoPullback:
        def fit(self, X, Y): pass

    class Pulls(NoPullback):
        def pullback_policy(self, *a, **k): pass
        def pullback_chain(self, *a, **k): pass

    def fitted(method, gold=g):
        pt = PolicyTransportation(method, verbose=False)
        pt.fit(gold["source"], gold["target"])
        return pt

    with pytest.raises(ValueError, match="1 .. 4 transports, got 0"):
        TransportChain([])
    with pytest.raises(ValueError, match="1 .. 4 transports, got 5"):
        TransportChain([fitted(Pulls()) for _ in range(5)])
    with pytest.raises(RuntimeError, match="transport 1 is not fitted"):
        TransportChain([fitted(Pulls()), GaussianProcessTransportation(optimizer=None, verbose=False)])
    with pytest.raises(ValueError, match=r"share one space.*\[2, 3\]"):
        TransportChain([fitted(Pulls()), fitted(Pulls(), g3)])
    with pytest.raises(NotImplementedError, match="transport 1 .NoPullback."):
        TransportChain([fitted(Pulls()), fitted(NoPullback())])
    chain = TransportChain([fitted(Pulls()), fitted(Pulls())], verbose=False)
    assert len(chain) == 2 and chain.n_features == 2
    with pytest.raises(TypeError, match="tolerance"):
        chain.transported_policy(None, g["traj"][:2], tolerance=1.0)
    # GaussianProcess.pullback_chain itself: counts and unfitted members before anything touches a device
    gp = [GaussianProcess(kernel=sk_kernel(0.1, [0.3], 1e-3), optimizer=None, verbose=False) for _ in range(6)]
    with pytest.raises(ValueError, match="1 .. 4 maps, got 5"):
        gp[0].pullback_chain(gp[1:5], gp[5], np.zeros((2, 2)), [None] * 5)
    with pytest.raises(ValueError, match="2 maps, 1 affine"):
        gp[0].pullback_chain(gp[1:2], gp[5], np.zeros((2, 2)), [None])
    with pytest.raises(RuntimeError, match="not fitted"):
        gp[0].pullback_chain(gp[1:2], gp[5], np.zeros((2, 2)), [None] * 2)


# ------------------------------------------------------------------------------------------------------------ GPU
def _fit_rings(centre, nu=None, push=(2.0, 0.5, 0.0), do_scale=False):
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    tr = GaussianProcessTransportation(kernel_transport=sk_kernel(4.0, [6.0, 6.0], 1e-3, nu), optimizer=None, verbose=False,
                                       matern_derivatives=nu is not None)
    tr.source_distribution, tr.target_distribution = rings(centre, push)
    tr.fit_transportation(do_scale=do_scale)
    return tr


def _case(transports, gp_dyn, nus, nu_dyn=None):
    maps = [t.method.delta_map for t in transports]
    return {"tr": transports, "maps": maps, "affs": [_affine_of(t) for t in transports], "gp_dyn": gp_dyn, "nus": nus,
            "models": [_model_of(m, nu) for m, nu in zip(maps, nus)], "dyn_model": _model_of(gp_dyn, nu_dyn)}


def _chain_call(case, y, x0=None, outputs=None, rtol=RTOL, max_passes=64, std_offset=None, K=None):
    from gaussian_process_transportation_amd import _lib
    maps, affs = case["maps"][:K], case["affs"][:K]
    off = np.sqrt(case["gp_dyn"]._noise) if std_offset is None else std_offset
    stages = [(m._handle, a["R"], a["c_src"], a["c_dst"], a["scale"], a.get("R_jac")) for m, a in zip(maps, affs)]
    return maps[-1]._handle.pullback_chain(stages, case["gp_dyn"]._handle, y, x0=x0, rtol=rtol, max_passes=max_passes, std_offset=off,
                                           outputs=_lib.CHAIN_OUTPUTS if outputs is None else outputs)


def _cascade(case, y, max_passes=64, K=None):
    """gpt_pullback_policy per stage, the last stage first, x of one the y of the next."""
    maps, affs = case["maps"][:K], case["affs"][:K]
    per, yk = [None] * len(maps), y
    for k in range(len(maps) - 1, -1, -1):
        per[k] = _call(maps[k], case["gp_dyn"], yk, affs[k], max_passes=max_passes)
        yk = np.ascontiguousarray(per[k]["x"])
    return per


def _check_against_cascade(what, case, y, max_passes=64, K=None):
    K = len(case["maps"]) if K is None else K
    out, per = _chain_call(case, y, max_passes=max_passes, K=K), _cascade(case, y, max_passes, K)
    print(f"{what}: status per stage {[list(_counts(s)) for s in out['stage_status']]}, passes <= {out['stage_passes'].max(axis=1)}")
    for name, key in (("stage_z", "post_z"), ("stage_x", "x"), ("stage_A", "post_A"), ("stage_status", "status"), ("stage_passes", "passes"),
                      ("stage_residual", "residual"), ("stage_det", "det")):
        for k in range(K):
            assert out[name][k].tobytes() == per[k][key].tobytes(), (what, name, k)
    assert out["f"].tobytes() == per[0]["f"].tobytes() and out["x"].tobytes() == per[0]["x"].tobytes(), what
    exact, tol = CH.velocity(case["affs"][:K], out["f"], out["stage_A"])
    err = np.abs(out["vel"].astype(LD) - exact)
    print(f"{what}: vel largest share of 16 (K + 1) eps S {float(np.max(err / tol)):.3f}")
    assert np.all(err <= tol), what
    assert np.array_equal(out["status"], CH.first_failing(out["stage_status"])), what
    return out, per


@pytest.fixture(scope="module")
def letter2():
    """The two-stage fixture of the module docstring on the device, and its grid."""
    g = load_golden("letterS_2d")
    tr0 = _fit_transport(g)
    tr1 = _fit_rings(g["traj"][200])
    dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01)
    return dict(_case([tr0, tr1], dyn, [None, None]), g=g, grid=box_grid(g["traj"]))


@pytest.fixture(scope="module")
def letter3():
    """A do_scale=True first stage, the rings, a Matern 5/2 stage with its analytic derivatives, and a Matern 1/2 dynamics."""
    g = load_golden("letterS_2d")
    tr0 = _fit_transport(g, do_scale=True)
    tr1 = _fit_rings(g["traj2"][200])
    tr2 = _fit_rings(g["traj2"][100], nu=2.5, push=(1.0, 0.25, 0.0))
    dyn = _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01, 0.5)
    return dict(_case([tr0, tr1, tr2], dyn, [None, None, 2.5], 0.5), g=g, grid=box_grid(g["traj2"]))


@pytest.mark.gpu
def test_single_stage_is_gpt_pullback_policy(letter2):
    """K = 1: every shared output bit for bit, with and without a guess, stalled points included; the variances to the bound."""
    case, g = letter2, letter2["g"]
    for y, x0 in ((np.ascontiguousarray(np.concatenate([case["grid"], g["traj"][::9]])), None), (np.ascontiguousarray(g["traj"][::5]), g["demo"][::5])):
        one = _chain_call(case, y, x0=x0, K=1)
        ref = _call(case["maps"][0], case["gp_dyn"], y, case["affs"][0], x0=x0)
        for k in ("x", "vel", "f", "status"):
            assert one[k].tobytes() == ref[k].tobytes(), k
        for k, r in (("stage_det", "det"), ("stage_residual", "residual"), ("stage_passes", "passes"), ("stage_status", "status"),
                     ("stage_z", "post_z"), ("stage_A", "post_A"), ("stage_x", "x")):
            assert one[k].shape[0] == 1 and one[k][0].tobytes() == ref[r].tobytes(), k
        if x0 is None:
            assert np.any(ref["status"] == INV.STALLED)
        v = CH.variances(case["affs"][:1], one["f"], one["stage_A"], one["var_dyn"], one["stage_Jvar"], np.sqrt(case["gp_dyn"]._noise))
        assert np.all(np.abs(one["vel_var_dyn"] - ref["vel_var_dyn"]) <= np.asarray(v["vel_var_dyn"][1], dtype=float))
        for i in range(2):
            assert np.all(np.abs(one["vel_var_map"][:, i] - ref["vel_var_map"]) <= np.asarray(v["vel_var_map"][1][:, i], dtype=float))


@pytest.mark.gpu
def test_two_stages_against_the_cascade(letter2):
    case = letter2
    y = np.ascontiguousarray(np.concatenate([case["grid"], case["g"]["traj"][::7]]))
    out, _ = _check_against_cascade("letterS + rings", case, y)
    assert np.all(out["stage_status"][1] == INV.CONVERGED)
    stalled = out["stage_status"][0] == INV.STALLED
    assert np.any(stalled) and np.all(out["status"][stalled] == INV.STALLED)      # a stage that did not converge: the rest still ran
    assert np.all(np.isfinite(out["vel"])) and np.all(np.isfinite(out["x"]))
    for max_passes in (1, 3):                                                      # MAX_PASSES at the last stage: the stages before it still run
        out, _ = _check_against_cascade(f"letterS + rings max_passes={max_passes}", case, y, max_passes=max_passes)
        assert np.any(out["stage_status"][1] == INV.MAX_PASSES) and np.all(out["stage_passes"] <= max_passes)


@pytest.mark.gpu
def test_three_stages_against_the_cascade(letter3):
    case = letter3
    y = np.ascontiguousarray(np.concatenate([case["grid"], case["g"]["traj2"][::7]]))
    out, _ = _check_against_cascade("letterS do_scale + rings + Matern 5/2 rings, Matern 1/2 dynamics", case, y)
    assert len(set(out["status"])) >= 2                                           # (the launch holds queries that end differently)


def _synthetic_stage(points, k, ls):
    """A small smooth displacement on `points`: invertible, one Newton basin."""
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    span = np.ptp(points, axis=0).max()
    tr = GaussianProcessTransportation(kernel_transport=sk_kernel(0.1 * span ** 2, [ls * span] * points.shape[1], 1e-4), optimizer=None, verbose=False)
    tr.source_distribution = points
    tr.target_distribution = points + 0.02 * span * np.sin(3.0 * (points - points.mean(axis=0)) / span + k)
    tr.fit_transportation()
    return tr


@pytest.mark.gpu
def test_four_stages_3d():
    """K = GPT_CHAIN_MAX at D = 3, M = 5: surface_3d with its sources cut to 100 and three small synthetic displacements."""
    from gaussian_process_transportation_amd import TransportChain
    g = load_golden("surface_3d")
    tr0 = _fit_transport(dict(g, source=g["source"][:100], target=g["target"][:100]))
    rng = np.random.default_rng(11)
    moved = tr0.method.transport(g["demo"], return_std=False)[0]
    lo, hi = moved.min(axis=0), moved.max(axis=0)
    trs = [tr0] + [_synthetic_stage(rng.uniform(lo, hi, (40 + 13 * k, 3)), k, 0.4) for k in range(1, 4)]
    dyn = _fit_gp(g["demo"], g["delta"], 0.05, [0.5, 0.6, 0.7], 1e-4, 1.5)
    case = _case(trs, dyn, [None] * 4, 1.5)
    X = np.ascontiguousarray(g["demo"][::len(g["demo"]) // 5][:5])
    y = np.ascontiguousarray(TransportChain(trs, verbose=False).transport(X)[0])
    out, _ = _check_against_cascade("surface_3d + 3 synthetic stages", case, y)
    assert out["stage_x"].shape == (4, 5, 3) and out["stage_A"].shape == (4, 5, 3, 3)
    guessed = _chain_call(case, y, x0=X)
    assert np.all(guessed["stage_passes"] == 1) and np.all(guessed["status"] == INV.CONVERGED)
    _check_variances("surface_3d + 3 synthetic stages", case, guessed)


@pytest.mark.gpu
def test_two_stages_1d():
    a, b = _synthetic_case(1, 64, 100, None, 1.5), _synthetic_case(1, 40, 1, 2.5, None, seed=5)
    case = {"maps": [a["gp_map"], b["gp_map"]], "affs": [a["aff"], b["aff"]], "gp_dyn": a["gp_dyn"], "nus": [None, 2.5],
            "models": [a["map_model"], b["map_model"]], "dyn_model": a["dyn_model"]}
    y = np.ascontiguousarray(b["aff"]["c_dst"] + np.array([[-0.2], [0.05], [0.25]]))
    out, _ = _check_against_cascade("1-D, RBF + Matern 5/2", case, y)
    assert out["vel"].shape == (3, 1) and out["stage_A"].shape == (2, 3, 1, 1)
    _check_variances("1-D", case, out)


@pytest.mark.gpu
def test_known_preimage(letter2):
    from gaussian_process_transportation_amd import TransportChain
    case, g = letter2, letter2["g"]
    chain = TransportChain(case["tr"], verbose=False)
    X = np.ascontiguousarray(g["demo"][::8])
    y, vel_fwd, _, stds = chain.transport(X, vel=g["delta"][::8])
    assert len(stds) == 2 and y.shape == X.shape and vel_fwd.shape == X.shape
    out = _chain_call(case, np.ascontiguousarray(y), x0=X)
    assert np.all(out["status"] == INV.CONVERGED) and np.all(out["stage_passes"] == 1)
    bound = CH.carried_bound(case["models"], case["affs"], out["stage_z"], [out["stage_x"][1], y], RTOL)
    err = np.linalg.norm(out["x"] - X, axis=1)
    print(f"known preimage: |x - X| <= {err.max():.2e}, largest share of the carried bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # the Python level: the same call through TransportChain, the forward velocities of the demonstration back as the policy at y
    vel, std, info = chain.transported_policy(case["gp_dyn"], y, x0=X, return_std=True, return_info=True, rtol=RTOL)
    assert vel.tobytes() == out["vel"].tobytes() and info["x"].tobytes() == out["x"].tobytes()
    assert std.shape == vel.shape and np.all(np.isfinite(std)) and np.all(std >= 0)
    assert np.allclose(std ** 2, out["vel_var_dyn"] + out["vel_var_map"], rtol=1e-9, atol=0)
    x_inv, inv = chain.inverse_transport(y, x0=X, return_info=True, rtol=RTOL)
    assert x_inv.tobytes() == out["x"].tobytes() and inv["stage_passes"].tobytes() == out["stage_passes"].tobytes()
    assert chain.transported_policy(case["gp_dyn"], y, x0=X, rtol=RTOL).tobytes() == vel.tobytes()


@pytest.mark.gpu
def test_independence_of_M_and_order(letter2):
    case = letter2
    base = np.ascontiguousarray(np.concatenate([case["grid"][150:170], case["g"]["traj"][::23]]))[:37]
    full = _chain_call(case, base)
    for M in (1, 4, 5):
        part = _chain_call(case, base[:M])
        for k in ONE_LAUNCH:
            sl = full[k][:, :M] if k.startswith("stage_") else full[k][:M]
            assert part[k].tobytes() == np.ascontiguousarray(sl).tobytes(), (M, k)
    perm = np.random.default_rng(3).permutation(len(base))
    mixed = _chain_call(case, np.ascontiguousarray(base[perm]))
    for k in ONE_LAUNCH:
        want = full[k][:, perm] if k.startswith("stage_") else full[k][perm]
        assert mixed[k].tobytes() == np.ascontiguousarray(want).tobytes(), k


def _check_variances(what, case, out):
    K = len(case["maps"])
    gp_dyn = case["gp_dyn"]
    D = out["x"].shape[1]
    ref_d = gp_dyn._handle.predict_all(out["x"], var=True)["var"]
    assert np.all(np.abs(out["var_dyn"] - ref_d) <= VAR_SPLIT_RTOL * gp_dyn._c), what
    for k, (gp, nu) in enumerate(zip(case["maps"], case["nus"])):
        ref = gp._handle.predict_all(np.ascontiguousarray(out["stage_z"][k]), var=True, Jvar=True)
        prior_j = gp._c * G0[nu] / np.broadcast_to(gp._ls, (D,)) ** 2
        assert np.all(np.abs(out["stage_map_var"][k] - ref["var"]) <= VAR_SPLIT_RTOL * gp._c), (what, k)
        assert np.all(np.abs(out["stage_Jvar"][k] - ref["Jvar"]) <= VAR_SPLIT_RTOL * prior_j[None]), (what, k)
    v = CH.variances(case["affs"], out["f"], out["stage_A"], out["var_dyn"], out["stage_Jvar"], np.sqrt(gp_dyn._noise))
    for name in ("vel_var_map", "vel_var_dyn"):
        exact, tol = v[name]
        err = np.abs(out[name].astype(LD) - exact)
        share = np.divide(err, tol, out=np.zeros_like(err), where=tol > 0)
        print(f"{what}: {name} largest share of 16 (K + 1) eps S {float(np.max(share)):.3f} (K = {K})")
        assert np.all(err <= tol), (what, name)


@pytest.mark.gpu
def test_variances(letter2, letter3):
    for what, case, T in (("two stages", letter2, letter2["g"]["traj"]), ("three stages", letter3, letter3["g"]["traj2"])):
        y = np.ascontiguousarray(np.concatenate([case["grid"][::9], T[::11]]))
        out = _chain_call(case, y)
        _check_variances(what, case, out)
        # "vel" alone: the same one launch; the variance launches of the maps have three columns, not four
        few = _chain_call(case, y, outputs=("vel_var_map", "vel_var_dyn"))
        assert set(few) == {"vel", "status", "vel_var_map", "vel_var_dyn"} and few["vel"].tobytes() == out["vel"].tobytes()
        v = CH.variances(case["affs"], out["f"], out["stage_A"], out["var_dyn"], out["stage_Jvar"], np.sqrt(case["gp_dyn"]._noise))
        assert np.all(np.abs(few["vel_var_dyn"] - out["vel_var_dyn"]) <= np.asarray(v["vel_var_dyn"][1], dtype=float))


def _shapes(K, M, D):
    return {"x": (M, D), "vel": (M, D), "f": (M, D), "status": (M,), "var_dyn": (M,), "vel_var_map": (M, D), "vel_var_dyn": (M, D),
            "stage_x": (K, M, D), "stage_z": (K, M, D), "stage_A": (K, M, D, D), "stage_Jvar": (K, M, D), "stage_map_var": (K, M),
            "stage_status": (K, M), "stage_passes": (K, M), "stage_residual": (K, M), "stage_det": (K, M)}


def _sentinels(K, M, D):
    from gaussian_process_transportation_amd import _lib
    return {k: (np.full(s, ISENT, dtype=np.int32) if k in _lib.CHAIN_INT_OUTPUTS else np.full(s, SENT)) for k, s in _shapes(K, M, D).items()}


def _raw(stages, hd, M, y, x0, outs, K=None, rtol=RTOL, max_passes=64, std_offset=0.1, entry="gpt_pullback_chain"):
    """The C entry point itself on numpy arrays.  stages: [(handle or None, R, c_src, c_dst, scale, R_jac)] or None; outs: name ->
    array or None.  Returns (rc, message)."""
    from gaussian_process_transportation_amd import _lib
    C = _lib.C
    addr = lambda a: None if a is None else a.ctypes.data      # (the arrays live in the caller's tuples until the call returns)
    arr = None
    if stages is not None:
        arr = (_lib.ChainStage * max(1, len(stages)))()
        for k, (h, R, c_src, c_dst, scale, R_jac) in enumerate(stages):
            arr[k] = _lib.ChainStage(None if h is None else h._h, addr(R), addr(c_src), addr(c_dst), addr(R_jac), float(scale))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
    ptr = lambda k: ip(outs.get(k)) if k in _lib.CHAIN_INT_OUTPUTS else _lib.dptr(outs.get(k))
    y_, x0_ = _lib.dptr(y), _lib.dptr(x0)
    if entry.endswith("_dev"):                     # (every refusal asked of the device entry comes before it looks at an array)
        ptr, y_, x0_ = (lambda k: None), None, None
    rc = getattr(_lib.load(), entry)(arr, len(stages) if K is None else K, None if hd is None else hd._h, y_, x0_, M, float(rtol), int(max_passes),
                                     float(std_offset), *(ptr(k) for k in _lib.CHAIN_OUTPUTS))
    return rc, _lib.last_error()


def _stage_tuples(case, K=None):
    return [(m._handle, a["R"], a["c_src"], a["c_dst"], a["scale"], a.get("R_jac", a["R"])) for m, a in zip(case["maps"][:K], case["affs"][:K])]


def _mixed_rows(case):
    """134 rows on the moved demonstration and 100 of the grid, stalled points among them."""
    return np.ascontiguousarray(np.concatenate([case["g"]["traj"][::3], case["grid"][::4]]))


@pytest.mark.gpu
def test_optional_outputs(letter2):
    from gaussian_process_transportation_amd import _lib
    case = letter2
    hd, stages = case["gp_dyn"]._handle, _stage_tuples(case)
    off = np.sqrt(case["gp_dyn"]._noise)
    base = _mixed_rows(case)
    small = _chain_call(case, base)
    # only vel and status asked for: nothing else is written; rows past M stay sentinels
    few = _sentinels(2, 7, 2)
    rc, msg = _raw(stages, hd, 5, base[:5], None, {k: few[k] for k in ("vel", "status")}, std_offset=off)
    assert rc == _lib.GPT_OK, msg
    assert all(_untouched(v) for k, v in few.items() if k not in ("vel", "status"))
    assert few["vel"][:5].tobytes() == small["vel"][:5].tobytes() and _untouched(few["vel"][5:]) and _untouched(few["status"][5:])
    # each optional output alone
    for name in _lib.CHAIN_OUTPUTS:
        if name in ("vel", "status"):
            continue
        one = _chain_call(case, base[:9], outputs=(name,))
        assert set(one) == {"vel", "status", name}
        if name in ONE_LAUNCH:
            sl = small[name][:, :9] if name.startswith("stage_") else small[name][:9]
            assert one[name].tobytes() == np.ascontiguousarray(sl).tobytes(), name


@pytest.mark.gpu
def test_host_chunk_boundary(letter2):
    """M = HOST_CHUNK + 1 at N = 20 / 36 walks both staging sets: the rows round the boundary and the tail against a small call,
    the stage-major arrays included; the periodic input comes back periodic."""
    case = letter2
    base = _mixed_rows(case)
    small = _chain_call(case, base, outputs=ONE_LAUNCH)
    M = HOST_CHUNK + 1
    y = np.ascontiguousarray(np.tile(base, (-(-M // len(base)), 1))[:M])
    names = ("x", "f", "stage_x", "stage_z", "stage_A", "stage_status", "stage_passes", "stage_residual", "stage_det")
    big = _chain_call(case, y, outputs=names)
    rows = np.r_[0:len(base), HOST_CHUNK - len(base):HOST_CHUNK + 1]
    for k in ONE_LAUNCH:
        got = big[k][:, rows] if k.startswith("stage_") else big[k][rows]
        want = small[k][:, rows % len(base)] if k.startswith("stage_") else small[k][rows % len(base)]
        assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), k
    assert big["vel"][:len(base)].tobytes() == big["vel"][len(base):2 * len(base)].tobytes()


@pytest.mark.gpu
def test_device_entry(letter2):
    """gpt_pullback_chain_dev on torch tensors equals the host entry."""
    import torch
    from gaussian_process_transportation_amd import _lib
    case = letter2
    hd, off = case["gp_dyn"]._handle, np.sqrt(case["gp_dyn"]._noise)
    base = _mixed_rows(case)
    small = _chain_call(case, base)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    keep = [[t(a["R"]), t(a["c_src"]), t(a["c_dst"])] for a in case["affs"]]
    dstages = [(m._handle, R.data_ptr(), cs.data_ptr(), cd.data_ptr(), a["scale"], R.data_ptr()) for m, a, (R, cs, cd) in zip(case["maps"], case["affs"], keep)]
    yd = t(base)
    sent = _sentinels(2, len(base), 2)
    outs = {k: torch.from_numpy(v).to(dev) for k, v in sent.items()}
    h_last = case["maps"][-1]._handle
    h_last.pullback_chain_dev(dstages, hd, yd.data_ptr(), len(base), outs["vel"].data_ptr(), outs["status"].data_ptr(), rtol=RTOL, std_offset=off,
                              **{k + "_ptr": v.data_ptr() for k, v in outs.items() if k not in ("vel", "status")})
    h_last.synchronize()
    for k in _lib.CHAIN_OUTPUTS:
        assert outs[k].cpu().numpy().tobytes() == small[k].tobytes(), k                 # (the same launches at the same M, variances included)
    part = {k: torch.from_numpy(v).to(dev) for k, v in _sentinels(2, len(base), 2).items()}
    h_last.pullback_chain_dev(dstages, hd, yd.data_ptr(), len(base), part["vel"].data_ptr(), part["status"].data_ptr(), rtol=RTOL, std_offset=off,
                              stage_det_ptr=part["stage_det"].data_ptr())
    h_last.synchronize()
    assert part["vel"].cpu().numpy().tobytes() == small["vel"].tobytes() and part["stage_det"].cpu().numpy().tobytes() == small["stage_det"].tobytes()
    assert all(_untouched(v.cpu().numpy()) for k, v in part.items() if k not in ("vel", "status", "stage_det"))


@pytest.mark.gpu
def test_refusals_and_models_untouched(letter2):
    from gaussian_process_transportation_amd import _lib
    case = letter2
    hd, stages = case["gp_dyn"]._handle, _stage_tuples(case)
    y = np.ascontiguousarray(case["g"]["traj"][:4])
    probes = [m._handle for m in case["maps"]] + [hd]
    before = [h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd) for h in probes]
    _chain_call(case, y)
    outs = _sentinels(2, 4, 2)

    def refused(match, st=stages, hhd=hd, M=4, y_=y, x0_=None, drop=(), code=_lib.GPT_E_ARG, dev=False, **kw):
        for entry in ("gpt_pullback_chain",) + (("gpt_pullback_chain_dev",) if dev else ()):
            rc, msg = _raw(st, hhd, M, y_, x0_, {k: v for k, v in outs.items() if k not in drop}, entry=entry, **kw)
            assert rc == code and match in msg, (entry, match, rc, msg)
        assert all(_untouched(v) for v in outs.values()), match

    swap = lambda k, **f: [tuple(f.get(n, v) for n, v in zip(("h", "R", "c_src", "c_dst", "scale", "R_jac"), s)) if i == k else s for i, s in enumerate(stages)]
    # K and the stages array
    refused("K must be 1 .. 4", K=0, dev=True)
    refused("K must be 1 .. 4", K=5, dev=True)
    refused("stages must not be NULL", st=None, K=2, dev=True)
    # handles: NULL, unfitted, the same twice
    refused("NULL handle (stage 0 map)", st=swap(0, h=None), dev=True)
    refused("NULL handle (dynamics)", hhd=None, dev=True)
    empty = _lib.Handle(0)
    refused("stage 1 map model is not fitted", st=swap(1, h=empty), code=_lib.GPT_E_STATE, dev=True)
    refused("dynamics model is not fitted", hhd=empty, code=_lib.GPT_E_STATE, dev=True)
    refused("stages 0 and 1 are the same handle", st=swap(1, h=stages[0][0]), dev=True)
    refused("stage 1 and h_dyn are the same handle", hhd=stages[1][0], dev=True)
    for name in ("R", "c_src", "c_dst", "R_jac"):
        refused("must not be NULL (stage 1)", st=swap(1, **{name: None}), dev=True)
    if _lib.load().gpt_device_count() >= 2:
        other = _lib.Handle(1)
        other.fit(case["maps"][0].X, case["maps"][0].Y, np.full(2, 6.0), 4.0, 1e-3, 1e-10)
        refused("different devices", st=swap(0, h=other), dev=True)
        other.close()
    # per handle what gpt_pullback_policy refuses, with the stage in the message
    rng = np.random.default_rng(0)
    X2, X3 = rng.uniform(0, 1, (30, 2)), rng.uniform(0, 1, (30, 3))
    three_d = _fit_gp(X3, 0.05 * np.sin(X3), 0.1, [0.3], 1e-3)
    refused("share one space", st=swap(0, h=three_d._handle), dev=True)
    refused("share one space", hhd=three_d._handle, dev=True)
    two_out = _fit_gp(X3, X3[:, :2], 0.1, [0.3], 1e-3)
    refused("the stage 0 map model must map a space onto itself", st=swap(0, h=two_out._handle))
    f32 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, [0.3], 1e-3, dtype="float32")
    refused("fp64 models only (the stage 1 map", st=swap(1, h=f32._handle))
    refused("fp64 models only (the dynamics", hhd=f32._handle)
    m12 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, 0.3, 1e-3, 0.5, matern_derivatives=True)
    refused("Matern 1/2", st=swap(0, h=m12._handle))
    m52 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, 0.3, 1e-3, 2.5)
    refused("gpt_set_matern_derivatives", st=swap(1, h=m52._handle))
    rc, msg = _raw(stages, m12._handle, 4, y, None, {k: outs[k].copy() for k in ("vel", "status")})      # Matern dynamics are fine
    assert rc == _lib.GPT_OK, msg
    # the solver's arguments, M, required arrays
    for bad in (0.0, -1e-3, float("nan")):
        refused("rtol", rtol=bad, dev=True)
    refused("max_passes", max_passes=0, dev=True)
    refused("2^31", M=-1, dev=True)
    refused("2^31", M=2 ** 31, dev=True)
    refused("must not be NULL", y_=None)
    refused("must not be NULL", drop=("vel",))
    refused("must not be NULL", drop=("status",))
    # NaN or infinity in the host call's inputs
    nan_at = lambda a, i: np.ascontiguousarray(np.where(np.arange(a.size).reshape(a.shape) == i, np.nan, a))
    refused("NaN or infinity", y_=nan_at(y, 3))
    refused("NaN or infinity", x0_=nan_at(y, 0))
    refused("NaN or infinity", st=swap(0, scale=float("inf")))
    refused("NaN or infinity", st=swap(1, R=nan_at(stages[1][1], 2)))
    refused("NaN or infinity", st=swap(1, c_dst=np.full(2, np.nan)))
    refused("NaN or infinity", std_offset=float("nan"))
    # M = 0 does nothing
    rc, _ = _raw(stages, hd, 0, y, None, outs)
    assert rc == _lib.GPT_OK and all(_untouched(v) for v in outs.values())
    none = _chain_call(case, np.zeros((0, 2)))
    assert none["vel"].shape == (0, 2) and none["stage_A"].shape == (2, 0, 2, 2)
    empty.close()
    # every model predicts exactly what it did before the chain calls
    for h, was in zip(probes, before):
        now = h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd)
        for k in was:
            if was[k] is not None:
                assert was[k].tobytes() == now[k].tobytes(), k
