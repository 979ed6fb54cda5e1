"""The transport in one device call: gpt_transport_policy (csrc/gpt_transport.hip around the unchanged posterior launches),
_lib.Handle.transport_policy / transport_policy_dev, GaussianProcess.transport_policy, PolicyTransportation.transport_all and
GaussianProcessTransportation(fused=True).

Bounds.  The epilogue's outputs are sums of at most D + 1 fp64 products of its inputs; each is held to 16 eps S of its exact
(longdouble) value, S the same expression with absolute values on every product (transport_fused_restatement.epilogue).  The
quaternion is the dominant eigenvector v of Bar-Itzhack's 4 x 4 matrix K: residual |Kv - (v'Kv)v| <= 32 eps |K|_F, eigenvalue
lambda_max - v'Kv <= 32 eps |K|_F, ||v| - 1| <= 16 eps, and min|+-v - u_eigh| <= 64 eps |K|_F / gap where gap >= 1e-3 |K|_F.
A 6-sweep numpy Jacobi measured 8.3, 7.6, 5 and 6.2 against those four: they are 4 - 10 x what the algorithm does in fp64.
Variances of one query in launches of different size agree to 1e-11 of the prior variance (tests/test_gpu_parity.py, the
sharded prediction: the variance kernel's work split depends on M)."""
import numpy as np
import pytest

from tests import transport_fused_restatement as R
from tests.conftest import assert_parity, load_golden

EPS = np.finfo(np.float64).eps
LD = np.longdouble
SENT = -7.25e300
VAR_SPLIT_RTOL = 1e-11         # tests/test_gpu_parity.py::_two_rank_worker: |var - var'| <= 1e-11 max(var) between launch sizes
GOLDEN_RTOL = 1e-5             # tests/test_gpu_parity.py: RTOL of the unfused path against the same goldens


def sk_rbf(c, ls, noise):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    return ConstantKernel(float(c)) * RBF(length_scale=np.atleast_1d(np.asarray(ls, dtype=float)).tolist()) + WhiteKernel(float(noise))


def sk_matern(c, ls, nu, noise):
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel
    return ConstantKernel(c) * Matern(length_scale=ls, nu=nu) + WhiteKernel(noise)


def robot_orientations(M):
    """The 102 unit quaternions of the robot demo, tiled to M rows."""
    ori = load_golden("robot_demo_last")["training_ori"]
    return np.ascontiguousarray(np.resize(ori, (M, 4)))


# ------------------------------------------------------------------------------------------------------------ CPU
def _jacobian_set(kind, n=200_000):
    rng = np.random.default_rng(7 if kind == "near_identity" else 8)
    Jp = np.eye(3)[None] + 0.5 * rng.standard_normal((n, 3, 3))
    if kind == "scaled_per_entry":
        return Jp * 10.0 ** rng.uniform(-3, 3, (n, 3, 3))
    if kind == "scaled":
        # one factor per matrix: the bounds are relative to |K|_F, so this set asks for the same accuracy six decades up and
        # down.  (A factor per ENTRY is another population: one entry then dominates, K tends to +-|a|/3 twice over, and 3.5 %
        # of the set has no gap — the closest rotation is not determined — against the 1 % allowed.)
        Jp = Jp * 10.0 ** rng.uniform(-3, 3, (n, 1, 1))
    return Jp


@pytest.mark.parametrize("kind", ["near_identity", "scaled", "scaled_per_entry"])
def test_jacobi_eigenvector_bounds(kind):
    K = R.bar_itzhack_matrix(_jacobian_set(kind))
    v, lam, gap = R.jacobi_dominant(K)
    c = R.quaternion_checks(K, v)
    print(kind, {k: float(np.nanmax(c[k])) for k in ("residual", "eigenvalue", "norm", "vector")}, "left out", c["left_out"])
    assert np.all(c["residual"] <= 32) and np.all(c["eigenvalue"] <= 32) and np.all(c["norm"] <= 16)
    assert np.all(c["vector"][~np.isnan(c["vector"])] <= 64)
    if kind != "scaled_per_entry":       # (that population is 3.5 % without a gap: held to everything that does not depend on one)
        assert c["left_out"] <= 0.01
    assert np.all(np.abs(gap - c["gap"]) <= 64 * EPS)


def test_jacobi_leaves_with_nan_after_the_fixed_sweeps():
    Jp = np.eye(3)[None].repeat(3, axis=0)
    Jp[1, 0, 1] = np.nan
    q, gap = R.quaternion_closest(Jp)
    assert np.all(np.isnan(q[1])) and np.isnan(gap[1])
    assert np.array_equal(q[0], [1, 0, 0, 0]) and np.array_equal(q[2], [1, 0, 0, 0])     # the identity: K is diagonal, no rotation


class OraclePlugin:
    """A delta_map on the CPU oracle; `transport_policy` through the restatement, so that PolicyTransportation.transport_all
    and GaussianProcessTransportation(fused=True) run without a device."""

    def __init__(self, c, ls, noise):
        from oracle.gp_oracle import GaussianProcessOracle
        self.gp = GaussianProcessOracle(c, ls, noise)
        self.calls = 0
        self._memo = {}

    def fit(self, X, Y):
        self.gp.fit(X, Y)
        self._memo = {}

    def _once(self, what, x, compute):
        """The oracle's derivative at the surface demo's size takes seconds: each distinct evaluation is made once."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        key = (what, x.shape, x.tobytes())
        if key not in self._memo:
            self._memo[key] = compute(x)
        return self._memo[key]

    def predict(self, x, return_std=False):
        mean, std = self._once("predict", x, lambda q: self.gp.predict(q, return_std=True))
        return (mean.copy(), std.copy()) if return_std else mean.copy()

    def derivative(self, x, return_var=False):
        J, Jvar = self._once("derivative", x, lambda q: self.gp.derivative(q, return_var=True))
        return (J.copy(), Jvar.copy()) if return_var else J.copy()

    def transport_policy(self, x, rotation, scale, source_centroid, target_centroid, jacobian=None, vel=None, ori=None,
                         return_posterior=False):
        self.calls += 1
        x = np.asarray(x, dtype=np.float64)
        D = x.shape[1]
        rot = scale * ((x - source_centroid) @ rotation.T) + target_centroid
        mean, std = self.predict(rot, return_std=True)
        J, Jvar = self.derivative(rot, return_var=True)
        J_ori = self.derivative(x)
        Rj = rotation if jacobian is None else jacobian
        e = R.epilogue(x, rotation, scale, source_centroid, target_centroid, Rj, mean, vel, J, Jvar[:, 0, :], J_ori)
        f64 = lambda k: e[k][0].astype(np.float64)
        out = {"pos": f64("pos_out"), "pos_rot": f64("pos_rot"), "std": std}
        if vel is not None:
            out.update(vel=f64("vel_out"), vel_var=np.repeat(f64("vel_var")[:, None], D, axis=1), det_vel=f64("det_vel"))
        if ori is not None:
            q, gap = R.quaternion_closest(f64("J_phi")) if D == 3 else (None, None)
            out.update(ori=None if q is None else R.quaternion_multiply(q, np.asarray(ori, dtype=np.float64)), ori_gap=gap,
                       det_ori=f64("det_ori"))
        return out


def _host_case(name, thin=1, every=1):
    """A PolicyTransportation over the oracle at the golden theta (every `thin`-th source point), its inputs (every `every`-th
    row of the demonstration), and the host path's results."""
    from gaussian_process_transportation_amd.policy_transportation import PolicyTransportation
    g = load_golden(name)
    pt = PolicyTransportation(OraclePlugin(g["constant_value"], g["length_scale"], g["noise_level"]), verbose=False)
    pt.fit(g["source"][::thin], g["target"][::thin], do_scale=name == "letterS_2d")
    pos, vel, ori = g["demo"][::every], g["delta"][::every], robot_orientations(len(g["demo"]))[::every]
    traj, std = pt.transport(pos)
    v, vv = pt.transport_velocity(pos, vel)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):          # (the 2-D case prints the reference's two lines)
        o = pt.transport_orientation(pos, ori)
    return {"name": name, "pt": pt, "pos": pos, "vel": vel, "ori": ori, "host": (traj, std, v, vv, o)}


@pytest.fixture(scope="module", params=["letterS_2d", "surface_3d"])
def host_case(request):
    """(surface_3d: the oracle's derivative at N = 2500 works through subnormal kernel values, seconds per hundred rows — every
    second row of the 460 keeps the whole model and the whole length of the demonstration.)"""
    return _host_case(request.param, every=2 if request.param == "surface_3d" else 1)


@pytest.fixture(scope="module", params=["letterS_2d", "surface_3d_thin"])
def wiring_case(request):
    """The Python layers are the same at any model size: the 3-D case keeps every 25th of the 2500 source points."""
    return _host_case("letterS_2d") if request.param == "letterS_2d" else _host_case("surface_3d", thin=25)


def _quaternion_bound(J_phi):
    """64 eps |K|_F / gap per row (inf where the gap is below 1e-3 |K|_F): how far two dominant eigenvectors may be apart."""
    K = R.bar_itzhack_matrix(J_phi)
    w = np.linalg.eigvalsh(K)
    rel = (w[:, -1] - w[:, -2]) / np.sqrt(np.sum(K * K, axis=(1, 2)))
    return np.where(rel >= 1e-3, 64 * EPS / np.maximum(rel, 1e-300), np.inf)


def _quaternion_distance(a, b):
    """Row-wise |a - b|, up to the common sign where the rotation part's w is too close to 0 to fix it."""
    return np.minimum(np.linalg.norm(a - b, axis=1), np.linalg.norm(a + b, axis=1))


def test_restatement_agrees_with_the_host_path(host_case):
    pt, pos, vel, ori = host_case["pt"], host_case["pos"], host_case["vel"], host_case["ori"]
    traj, std, v, vv, o = host_case["host"]
    got = R.transport_all(pt, pos, vel, ori)
    assert_parity(got[0], traj, 1e-12, "positions")
    assert_parity(got[2], v, 1e-12, "velocities")
    if pos.shape[1] != 3:
        assert o is None and got[4] is None
        return
    aff = pt.affine_transform
    J_phi = (np.eye(3) + pt.delta_map.derivative(pos)) @ aff.rotation_matrix
    bound = _quaternion_bound(J_phi)
    dist = _quaternion_distance(got[4], o)
    print("quaternions: largest share of the bound", float(np.max(dist / bound)), "rows without a bound", int(np.sum(np.isinf(bound))))
    assert np.mean(np.isinf(bound)) <= 0.01
    assert np.all(dist <= bound)


def test_transport_all_wiring_on_the_host(wiring_case, capsys):
    """PolicyTransportation.transport_all and GaussianProcessTransportation(fused=True) over a delta_map with transport_policy."""
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    from gaussian_process_transportation_amd.policy_transportation import PolicyTransportation
    pt, pos, vel, ori = wiring_case["pt"], wiring_case["pos"], wiring_case["vel"], wiring_case["ori"]
    traj, std, v, vv, o = wiring_case["host"]
    D = pos.shape[1]
    capsys.readouterr()
    got = pt.transport_all(pos, vel, ori, return_info=True)
    said = capsys.readouterr().out
    assert ("Robot orientation is not transported" in said) == (D != 3) and "diffeomorphic" not in said
    assert len(got) == 6 and {"det_vel", "det_ori", "pos_rot"} <= set(got[5])
    assert_parity(got[0], traj, 1e-12, "positions")
    assert_parity(got[1], std, 1e-9, "std")              # (the same posterior at positions that differ by rounding)
    assert_parity(got[2], v, 1e-12, "velocities")
    assert_parity(got[3], vv, 1e-9, "velocity variance")
    assert (got[4] is None) == (D != 3)
    just_pos = pt.transport_all(pos)
    assert just_pos[2] is None and just_pos[3] is None and just_pos[4] is None and np.array_equal(just_pos[0], got[0])
    pt.verbose = True
    try:
        pt.transport_all(pos, vel, ori)
    finally:
        pt.verbose = False
    assert capsys.readouterr().out.count("Is the map locally diffeomorphic?") == 2

    class NoFused:
        def fit(self, X, Y): pass
    bare = PolicyTransportation(NoFused(), verbose=False)
    bare.affine_transform = pt.affine_transform
    with pytest.raises(NotImplementedError, match="transport_policy"):
        bare.transport_all(pos)
    for fused in (False, True):
        tr = GaussianProcessTransportation(optimizer=None, verbose=False, fused=fused)
        assert tr.fused is fused
        tr.method = pt
        tr.training_traj, tr.training_delta, tr.training_ori = pos, vel, ori
        before = pt.delta_map.calls
        tr.apply_transportation()
        capsys.readouterr()
        assert pt.delta_map.calls - before == (1 if fused else 0)
        assert tr.training_traj_old is pos
        assert_parity(tr.training_traj, traj, 1e-12, "training_traj")
        assert_parity(tr.training_delta, v, 1e-12, "training_delta")
        assert tr.std.shape == std.shape and tr.var_vel_transported.shape == vv.shape
        assert (tr.training_ori is None) == (D != 3)
    assert GaussianProcessTransportation(optimizer=None, verbose=False).fused is False          # off unless asked for


def test_python_refusals_need_no_device():
    from gaussian_process_transportation_amd import GaussianProcess
    gp = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False)
    with pytest.raises(RuntimeError, match="not fitted"):
        gp.transport_policy(np.zeros((2, 3)), np.eye(3), 1.0, np.zeros(3), np.zeros(3))


# ------------------------------------------------------------------------------------------------------------ GPU
def _affine(D, seed=3):
    """A rotation, a scale != 1, centroids, and an R_jac that is neither R nor scale R (another rotation, its columns stretched
    by 1.2, 0.8, 1.1): an R read where R_jac belongs, or the two swapped, is an O(1) error in every velocity and orientation."""
    rng = np.random.default_rng(seed)

    def rotation():
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        if np.linalg.det(Q) < 0:
            Q[:, -1] *= -1
        return np.ascontiguousarray(Q)
    return {"R": rotation(), "scale": 1.0 + 0.3 * rng.uniform(), "c_src": rng.uniform(0.3, 0.7, D), "c_dst": rng.uniform(0.3, 0.7, D),
            "R_jac": np.ascontiguousarray(rotation() * np.array([1.2, 0.8, 1.1])[:D])}


def _call(h, pos, aff, vel=None, ori=None, outputs=None):
    from gaussian_process_transportation_amd import _lib
    return h.transport_policy(pos, aff["R"], aff["c_src"], aff["c_dst"], scale=aff["scale"], R_jac=aff.get("R_jac", aff["R"]), vel=vel, ori=ori,
                              outputs=_lib.TRANSPORT_OUTPUTS if outputs is None else outputs)


def _check_epilogue(what, out, pos, aff, vel, ori, post=None, extra=None):
    """Test 1: every output against its exact value from the epilogue's own inputs, the post_* arrays of `post` (default: of
    `out` itself).  extra: {name: absolute tolerance added to 16 eps S} for what is not the epilogue's own rounding."""
    post, extra = out if post is None else post, extra or {}
    e = R.epilogue(pos, aff["R"], aff["scale"], aff["c_src"], aff["c_dst"], aff.get("R_jac", aff["R"]), post["post_mean"], vel,
                   post["post_J"], post["post_Jvar"], post["post_J_ori"])
    for k in ("pos_rot", "pos_out", "vel_out", "vel_var", "det_vel", "det_ori"):
        if k not in out:
            assert vel is None and k in ("vel_out", "vel_var"), k
            continue
        exact, S = e[k]
        err = np.abs(out[k].astype(LD) - exact)
        tol = 16 * EPS * S + extra.get(k, 0.0)
        share = np.divide(err, tol, out=np.zeros_like(err), where=tol > 0)
        print(f"{what}: {k} largest share of 16 eps S{' + the variance split' if k in extra else ''}: {float(np.max(share)):.3f}")
        assert np.all(err <= tol), k
    if ori is None or pos.shape[1] != 3:
        assert "ori_out" not in out
        return
    J_phi = e["J_phi"][0]
    K = R.bar_itzhack_matrix(J_phi, LD)
    o = ori.astype(LD)
    inv = o * np.array([1, -1, -1, -1], dtype=LD) / np.sum(o * o, axis=1)[:, None]
    q = R.quaternion_multiply(out["ori_out"].astype(LD), inv)                  # the rotation the device applied, (w, x, y, z)
    assert np.all(q[:, 0] >= -8 * EPS)
    c = R.quaternion_checks(K, q[:, [1, 2, 3, 0]])
    print(f"{what}: quaternion residual {np.max(c['residual']):.2f} eigenvalue {np.max(c['eigenvalue']):.2f} norm {np.max(c['norm']):.2f} "
          f"eps; ori_gap error {np.max(np.abs(out['ori_gap'] - c['gap'])) / EPS:.2f} eps, smallest gap {c['gap'].min():.3f}")
    assert np.all(c["residual"] <= 32) and np.all(c["eigenvalue"] <= 32) and np.all(c["norm"] <= 16)
    assert np.all(np.abs(out["ori_gap"] - c["gap"]) <= 64 * EPS)


def _synthetic(kind):
    """The N = 64 model (RBF at the golden theta, or Matern with its analytic derivatives), its 48 queries and an affine part."""
    from gaussian_process_transportation_amd import GaussianProcess
    g = load_golden("synthetic_3d_N64")
    if kind == "rbf":
        gp = GaussianProcess(kernel=sk_rbf(g["constant_value"], g["length_scale"], g["noise_level"]), alpha=float(g["alpha"]), optimizer=None,
                             verbose=False).fit(g["X"], g["Y"])
    else:
        gp = GaussianProcess(kernel=sk_matern(0.1, np.array([0.3, 0.25, 0.35]), float(kind), 1e-4), optimizer=None, verbose=False,
                             matern_derivatives=True).fit(g["X"], g["Y"])
    rng = np.random.default_rng(5)
    M = len(g["Xq"])
    return {"gp": gp, "h": gp._handle, "pos": g["Xq"], "aff": _affine(3), "vel": rng.standard_normal((M, 3)), "ori": robot_orientations(M)}


@pytest.fixture(scope="module")
def syn():
    return _synthetic("rbf")


def _fit_transport(g, do_scale=False, **kw):
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    tr = GaussianProcessTransportation(kernel_transport=sk_rbf(g["constant_value"], g["length_scale"], g["noise_level"]), optimizer=None,
                                       verbose=False, **kw)
    tr.source_distribution, tr.target_distribution = g["source"], g["target"]
    tr.fit_transportation(do_scale=do_scale)
    return tr


def _affine_of(tr):
    a = tr.method.affine_transform
    return {"R": np.ascontiguousarray(a.rotation_matrix), "scale": float(a.scale), "c_src": a.S_centroid, "c_dst": a.T_centroid}


@pytest.fixture(scope="module")
def letter_gpu():
    g = load_golden("letterS_2d")
    tr = _fit_transport(g, do_scale=True)
    return {"g": g, "tr": tr, "h": tr.method.delta_map._handle, "aff": _affine_of(tr)}


@pytest.mark.gpu
@pytest.mark.parametrize("r_jac", ["is_R", "differs"])
def test_epilogue_on_its_own_inputs_3d(syn, r_jac):
    aff = dict(syn["aff"])
    if r_jac == "is_R":
        del aff["R_jac"]                          # the Python layer's choice: the unscaled rotation
    else:
        assert np.max(np.abs(aff["R_jac"] - aff["R"])) > 0.1 and np.max(np.abs(aff["R_jac"] - aff["scale"] * aff["R"])) > 0.1
    out = _call(syn["h"], syn["pos"], aff, syn["vel"], syn["ori"])
    _check_epilogue(f"synthetic_3d_N64, R_jac {r_jac}", out, syn["pos"], aff, syn["vel"], syn["ori"])
    if r_jac == "differs":                        # the jacobian= argument of the class reaches the same call
        got = syn["gp"].transport_policy(syn["pos"], aff["R"], aff["scale"], aff["c_src"], aff["c_dst"], jacobian=aff["R_jac"],
                                         vel=syn["vel"], ori=syn["ori"])
        assert got["vel"].tobytes() == out["vel_out"].tobytes() and got["ori"].tobytes() == out["ori_out"].tobytes()
        assert got["det_vel"].tobytes() == out["det_vel"].tobytes() and got["det_ori"].tobytes() == out["det_ori"].tobytes()


@pytest.mark.gpu
def test_epilogue_on_its_own_inputs_2d_scaled(letter_gpu):
    g, aff = letter_gpu["g"], letter_gpu["aff"]
    assert aff["scale"] != 1.0                                        # R != R_jac * scale matters
    out = _call(letter_gpu["h"], g["demo"], aff, g["delta"])
    assert "ori_out" not in out and "ori_gap" not in out
    _check_epilogue("letterS_2d", out, g["demo"], aff, g["delta"], None)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["syn", "letter"])
def test_the_posterior_it_consumed_is_the_librarys(which, syn, letter_gpu):
    if which == "syn":
        h, pos, out = syn["h"], syn["pos"], _call(syn["h"], syn["pos"], syn["aff"], syn["vel"], syn["ori"])
    else:
        h, pos = letter_gpu["h"], letter_gpu["g"]["demo"]
        out = _call(h, pos, letter_gpu["aff"], letter_gpu["g"]["delta"])
    ref = h.predict_all(out["pos_rot"], mean=True, var=True, J=True, Jvar=True)
    for k, r in (("post_mean", "mean"), ("var", "var"), ("post_J", "J"), ("post_Jvar", "Jvar")):
        print(which, k, "max difference", float(np.max(np.abs(out[k] - ref[r]))))
        assert out[k].tobytes() == ref[r].tobytes(), k
    at_pos = h.predict_all(pos, J=True)["J"]
    assert out["post_J_ori"].tobytes() == at_pos.tobytes()


@pytest.fixture(scope="module")
def surface_gpu():
    g = load_golden("surface_3d")
    return {"g": g, "tr": _fit_transport(g), "ori": robot_orientations(len(g["demo"]))}


def _apply(tr, g, ori, fused):
    tr.fused = fused
    tr.training_traj, tr.training_delta = g["demo"], g["delta"]
    tr.training_ori = ori
    tr.apply_transportation()
    return {k: getattr(tr, k) for k in ("training_traj", "std", "training_traj_old", "training_delta", "var_vel_transported", "training_ori")}


@pytest.mark.gpu
def test_surface_3d_goldens_fused(surface_gpu):
    g = surface_gpu["g"]
    got = _apply(surface_gpu["tr"], g, surface_gpu["ori"], fused=True)
    assert_parity(got["training_traj"], g["traj"], GOLDEN_RTOL, "traj")
    assert_parity(got["std"], g["std"], GOLDEN_RTOL, "std")
    assert_parity(got["training_delta"], g["vel"], GOLDEN_RTOL, "vel")
    assert_parity(got["var_vel_transported"], g["var_vel"], GOLDEN_RTOL, "var_vel")
    assert got["training_traj_old"] is g["demo"]


def _wiring(fused, unfused, ori):
    for k in ("training_traj", "std", "training_delta", "var_vel_transported"):
        assert_parity(fused[k], unfused[k], 1e-8, k)
    assert fused["training_traj_old"] is unfused["training_traj_old"]
    if fused["training_traj"].shape[1] != 3:
        assert fused["training_ori"] is None and unfused["training_ori"] is None
        return
    a, b = fused["training_ori"], unfused["training_ori"]
    assert a.shape == b.shape == ori.shape
    w = R.quaternion_multiply(b, ori * np.array([1.0, -1, -1, -1]))[:, 0]       # w of the rotation the unfused path applied
    firm = np.abs(w) >= 1e-6                                                   # its sign (w >= 0) is determined there
    print("quaternions: max difference", float(np.max(_quaternion_distance(a, b))), "rows with |w| < 1e-6:", int(np.sum(~firm)))
    assert np.all(np.linalg.norm(a - b, axis=1)[firm] <= 1e-8)
    assert np.all(_quaternion_distance(a, b) <= 1e-8)


@pytest.mark.gpu
def test_fused_against_unfused_surface_3d(surface_gpu):
    g, tr, ori = surface_gpu["g"], surface_gpu["tr"], surface_gpu["ori"]
    _wiring(_apply(tr, g, ori, fused=True), _apply(tr, g, ori, fused=False), ori)


@pytest.mark.gpu
def test_fused_against_unfused_letterS(letter_gpu):
    g, tr = letter_gpu["g"], letter_gpu["tr"]
    ori = robot_orientations(len(g["demo"]))
    _wiring(_apply(tr, g, ori, fused=True), _apply(tr, g, ori, fused=False), ori)


@pytest.mark.gpu
def test_chunk_boundary_and_optional_arrays(syn):
    h, aff = syn["h"], syn["aff"]
    g = load_golden("synthetic_3d_N64")
    M = 131072 + 1
    rng = np.random.default_rng(9)
    pos, vel, ori = rng.uniform(0, 1, (M, 3)), rng.standard_normal((M, 3)), robot_orientations(M)
    names = ("pos_rot", "pos_out", "var", "vel_out", "vel_var", "det_vel", "ori_out", "det_ori", "ori_gap")
    full = _call(h, pos, aff, vel, ori, outputs=names)
    rows = np.concatenate([[0, 131071, 131072], rng.choice(M, 32, replace=False)])
    # mean and J are computed per query, whatever M is: the separate call's post_* are the exact inputs of those rows of the
    # large call, whose outputs are therefore held to test 1's bounds themselves (16 eps S; the quaternion's residual,
    # eigenvalue and norm; ori_gap to 64 eps of numpy's).  Only the variance kernel's work split depends on M.
    sub = _call(h, pos[rows], aff, vel[rows], ori[rows])
    full_mean = h.predict_all(full["pos_rot"][rows], mean=True, J=True)
    assert full_mean["mean"].tobytes() == sub["post_mean"].tobytes() and full_mean["J"].tobytes() == sub["post_J"].tobytes()
    prior_dvar = float(g["constant_value"]) / float(np.min(g["length_scale"])) ** 2
    vr2 = lambda v: np.sum((np.abs(v) @ np.abs(aff["R_jac"]).T) ** 2, axis=1)
    at_rows = {k: v[rows] for k, v in full.items()}
    _check_epilogue("chunk boundary, rows of the M = 131073 call", at_rows, pos[rows], aff, vel[rows], ori[rows], post=sub,
                    extra={"vel_var": VAR_SPLIT_RTOL * prior_dvar * vr2(vel[rows])})
    dvar = np.abs(full["var"][rows] - sub["var"])
    print(f"chunk boundary: var max difference {dvar.max():.3e} of {VAR_SPLIT_RTOL * np.max(full['var']):.3e} allowed")
    assert np.all(dvar <= VAR_SPLIT_RTOL * np.max(full["var"]))
    for arr in full.values():
        assert np.all(np.isfinite(arr))
    # each of vel / ori absent, around a workgroup of k_push_forward's neighbours' sizes
    for m in (1, 63, 64, 65):
        both = _call(h, pos[:m], aff, vel[:m], ori[:m], outputs=names)
        for v_, o_ in ((None, ori[:m]), (vel[:m], None), (None, None)):
            got = _call(h, pos[:m], aff, v_, o_, outputs=names)
            gone = ({"vel_out", "vel_var"} if v_ is None else set()) | ({"ori_out"} if o_ is None else set())
            assert set(got) == set(names) - gone
            for k in got:
                if k in ("var", "vel_var"):              # the variance path differs with what is asked for
                    scale = np.max(both["var"]) if k == "var" else prior_dvar * vr2(vel[:m])
                    assert np.all(np.abs(got[k] - both[k]) <= VAR_SPLIT_RTOL * scale), (m, k)
                else:
                    assert got[k].tobytes() == both[k].tobytes(), (m, k)


@pytest.mark.gpu
@pytest.mark.parametrize("nu", ["1.5", "2.5"])
def test_matern_models(nu):
    s = _synthetic(nu)
    out = _call(s["h"], s["pos"], s["aff"], s["vel"], s["ori"])
    _check_epilogue(f"Matern nu={nu}", out, s["pos"], s["aff"], s["vel"], s["ori"])
    ref = s["h"].predict_all(out["pos_rot"], mean=True, var=True, J=True, Jvar=True)
    assert out["post_mean"].tobytes() == ref["mean"].tobytes() and out["post_J"].tobytes() == ref["J"].tobytes()
    got = s["gp"].transport_policy(s["pos"], s["aff"]["R"], s["aff"]["scale"], s["aff"]["c_src"], s["aff"]["c_dst"], jacobian=s["aff"]["R_jac"],
                                   vel=s["vel"], ori=s["ori"])
    assert got["pos"].tobytes() == out["pos_out"].tobytes() and got["ori"].tobytes() == out["ori_out"].tobytes()


def _raw(h, M, pos, aff, vel, ori, outs, entry="gpt_transport_policy"):
    """The C entry point itself on numpy arrays (`outs`: name -> array or None); returns (rc, message)."""
    from gaussian_process_transportation_amd import _lib
    p = _lib.dptr
    rc = getattr(h.lib, entry)(h._h, p(pos), M, p(aff["R"]), p(aff["c_src"]), p(aff["c_dst"]), float(aff["scale"]), p(aff.get("R_jac", aff["R"])), p(vel), p(ori),
                               *(p(outs.get(k)) for k in _lib.TRANSPORT_OUTPUTS))
    return rc, _lib.last_error()


def _sentinels(M, D):
    shapes = {"pos_rot": (M, D), "pos_out": (M, D), "var": (M,), "vel_out": (M, D), "vel_var": (M,), "det_vel": (M,), "ori_out": (M, 4),
              "det_ori": (M,), "ori_gap": (M,), "post_mean": (M, D), "post_J": (M, D, D), "post_Jvar": (M, D), "post_J_ori": (M, D, D)}
    return {k: np.full(s, SENT) for k, s in shapes.items()}


@pytest.mark.gpu
def test_refusals(syn, letter_gpu):
    from gaussian_process_transportation_amd import GaussianProcess, _lib
    h, pos, aff, vel, ori = syn["h"], syn["pos"][:4], syn["aff"], syn["vel"][:4], syn["ori"][:4]
    before = h.predict_all(syn["pos"], mean=True, var=True, J=True, Jvar=True)
    outs = _sentinels(4, 3)

    def refused(match, hh=h, M=4, pos_=pos, aff_=aff, vel_=vel, ori_=ori, drop=(), code=_lib.GPT_E_ARG):
        rc, msg = _raw(hh, M, pos_, aff_, vel_, ori_, {k: v for k, v in outs.items() if k not in drop})
        assert rc == code and match in msg, (rc, msg)
        for k, v in outs.items():
            assert np.all(v == SENT), (match, k)

    rng = np.random.default_rng(0)
    X3 = rng.uniform(0, 1, (50, 3))
    # D != O, D > 3
    two_out = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False).fit(X3, X3[:, :2])
    refused("D == O", hh=two_out._handle)
    with pytest.raises(NotImplementedError, match="onto itself"):
        two_out.transport_policy(pos, aff["R"], aff["scale"], aff["c_src"], aff["c_dst"])
    X4 = rng.uniform(0, 1, (50, 4))
    wide = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False).fit(X4, 0.05 * np.sin(X4))
    refused("D <= 3", hh=wide._handle)
    with pytest.raises(NotImplementedError, match="at most 3"):
        wide.transport_policy(X4[:3], np.eye(4), 1.0, np.zeros(4), np.zeros(4))
    # orientations of a 2-D model
    h2, aff2, pos2 = letter_gpu["h"], letter_gpu["aff"], letter_gpu["g"]["demo"][:4]
    outs2 = _sentinels(4, 2)
    for give in ({"pos_out", "ori_out"}, {"pos_out", "ori_gap"}, {"pos_out"}):
        rc, msg = _raw(h2, 4, pos2, aff2, None, ori, {k: v for k, v in outs2.items() if k in give})
        assert rc == _lib.GPT_E_ARG and "need D == 3" in msg
    assert all(np.all(v == SENT) for v in outs2.values())
    with pytest.raises(ValueError, match="need D == 3"):
        h2.transport_policy(pos2, aff2["R"], aff2["c_src"], aff2["c_dst"], ori=ori)
    # fp32 and multi-task models
    f32 = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False, dtype="float32").fit(X3, 0.05 * np.sin(X3))
    refused("fp64", hh=f32._handle)
    with pytest.raises(NotImplementedError, match="float64"):
        f32.transport_policy(pos, aff["R"], aff["scale"], aff["c_src"], aff["c_dst"])
    hs = _lib.Handle(0)
    refused("not fitted", hh=hs, code=_lib.GPT_E_STATE)
    hs.fit_svgp(X3, rng.standard_normal((3, 50)), 1e-2 * np.eye(50) * np.ones((3, 1, 1)), np.full(3, 0.3), np.ones(3))
    refused("single-task", hh=hs)
    hs.close()
    # Matern: 1/2 never, 3/2 and 5/2 only with the analytic derivatives enabled
    m12 = GaussianProcess(kernel=sk_matern(0.1, 0.3, 0.5, 1e-3), optimizer=None, verbose=False, matern_derivatives=True).fit(X3, 0.05 * np.sin(X3))
    refused("Matern 1/2", hh=m12._handle)
    with pytest.raises(NotImplementedError, match="nu=0.5"):
        m12.transport_policy(pos, aff["R"], aff["scale"], aff["c_src"], aff["c_dst"])
    for nu in (1.5, 2.5):
        m = GaussianProcess(kernel=sk_matern(0.1, 0.3, nu, 1e-3), optimizer=None, verbose=False).fit(X3, 0.05 * np.sin(X3))
        refused("gpt_set_matern_derivatives", hh=m._handle)
        with pytest.raises(NotImplementedError, match="matern_derivatives"):
            m.transport_policy(pos, aff["R"], aff["scale"], aff["c_src"], aff["c_dst"])
    # M out of range (both entry points), an output without its input, required arrays
    refused("2^31", M=-1)
    refused("2^31", M=2 ** 31)
    for M in (-1, 2 ** 31):
        rc, msg = _raw(h, M, None, {"R": None, "c_src": None, "c_dst": None, "scale": 1.0}, None, None, {}, entry="gpt_transport_policy_dev")
        assert rc == _lib.GPT_E_ARG and "2^31" in msg
    refused("need vel", vel_=None, drop=("vel_var",))
    refused("need vel", vel_=None, drop=("vel_out",))
    refused("needs ori", ori_=None)
    refused("must not be NULL", pos_=None)
    refused("must not be NULL", drop=("pos_out",))
    # NaN or infinity in the host call's inputs
    for bad in (dict(pos_=np.where(np.arange(12).reshape(4, 3) == 5, np.nan, pos)), dict(vel_=np.where(np.arange(12).reshape(4, 3) == 0, np.inf, vel)),
                dict(ori_=np.where(np.arange(16).reshape(4, 4) == 15, np.nan, ori)), dict(aff_=dict(aff, scale=float("nan"))),
                dict(aff_=dict(aff, R=np.where(np.eye(3) == 1, np.inf, aff["R"]))), dict(aff_=dict(aff, c_dst=np.full(3, np.nan)))):
        refused("NaN or infinity", **{k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in bad.items()})
    with pytest.raises(ValueError, match="NaN or infinity"):
        syn["gp"].transport_policy(np.full((2, 3), np.nan), aff["R"], aff["scale"], aff["c_src"], aff["c_dst"])
    # M = 0 does nothing
    rc, _ = _raw(h, 0, pos, aff, vel, ori, outs)
    assert rc == _lib.GPT_OK and all(np.all(v == SENT) for v in outs.values())
    empty = _call(h, np.zeros((0, 3)), aff)
    assert empty["pos_out"].shape == (0, 3)
    # the model and its scratch are as they were
    after = h.predict_all(syn["pos"], mean=True, var=True, J=True, Jvar=True)
    for k in before:
        if before[k] is not None:
            assert before[k].tobytes() == after[k].tobytes(), k


def _device_call(h, torch, dev, pos, aff, vel, ori, names):
    """gpt_transport_policy_dev on torch tensors; returns {name: tensor}."""
    M, D = pos.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    widths = {"pos_rot": (M, D), "pos_out": (M, D), "var": (M,), "vel_out": (M, D), "vel_var": (M,), "det_vel": (M,), "ori_out": (M, 4),
              "det_ori": (M,), "ori_gap": (M,), "post_mean": (M, D), "post_J": (M, D, D), "post_Jvar": (M, D), "post_J_ori": (M, D, D)}
    ins = {"pos": t(pos), "R": t(aff["R"]), "c_src": t(aff["c_src"]), "c_dst": t(aff["c_dst"]), "R_jac": t(aff.get("R_jac", aff["R"])), "vel": None if vel is None else t(vel),
           "ori": None if ori is None else t(ori)}
    outs = {k: torch.full(widths[k], SENT, dtype=torch.float64, device=dev) for k in names}
    ptr = lambda x: 0 if x is None else x.data_ptr()
    h.transport_policy_dev(ptr(ins["pos"]), M, ptr(ins["R"]), ptr(ins["c_src"]), ptr(ins["c_dst"]), aff["scale"], ptr(ins["R_jac"]),
                           outs["pos_out"].data_ptr(), vel_ptr=ptr(ins["vel"]), ori_ptr=ptr(ins["ori"]),
                           **{k + "_ptr": v.data_ptr() for k, v in outs.items() if k != "pos_out"})
    return outs, ins


@pytest.mark.gpu
def test_device_pointer_entry_on_a_callers_stream(syn):
    import torch
    from gaussian_process_transportation_amd import _lib
    h, pos, aff, vel, ori = syn["h"], syn["pos"], syn["aff"], syn["vel"], syn["ori"]
    host = _call(h, pos, aff, vel, ori)
    before = h.predict_all(pos, mean=True, var=True, J=True, Jvar=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    h.set_stream(stream.cuda_stream)
    try:
        every, keep1 = _device_call(h, torch, dev, pos, aff, vel, ori, _lib.TRANSPORT_OUTPUTS)
        stream.synchronize()
        few, keep2 = _device_call(h, torch, dev, pos, aff, vel, ori, ("pos_out", "vel_out", "ori_out"))     # the optional outputs left out
        stream.synchronize()
        bare, keep3 = _device_call(h, torch, dev, pos, aff, None, None, ("pos_out",))
        stream.synchronize()
    finally:
        h.set_stream(0)
    for k in _lib.TRANSPORT_OUTPUTS:
        assert every[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    for k in few:
        assert few[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    assert bare["pos_out"].cpu().numpy().tobytes() == host["pos_out"].tobytes()
    after = h.predict_all(pos, mean=True, var=True, J=True, Jvar=True)
    for k in before:
        if before[k] is not None:
            assert before[k].tobytes() == after[k].tobytes(), k


@pytest.mark.gpu
def test_nan_row_goes_through(syn):
    """A finite, bounded run: the Jacobi iteration has a fixed sweep count, so a NaN row leaves with NaN outputs like any other."""
    import torch
    from gaussian_process_transportation_amd import _lib
    h, aff, vel, ori = syn["h"], syn["aff"], syn["vel"], syn["ori"]
    pos = syn["pos"].copy()
    row = 17
    dev = torch.device("cuda", 0)
    clean, keep1 = _device_call(h, torch, dev, pos, aff, vel, ori, _lib.TRANSPORT_OUTPUTS)
    h.synchronize()
    pos[row] = np.nan
    dirty, keep2 = _device_call(h, torch, dev, pos, aff, vel, ori, _lib.TRANSPORT_OUTPUTS)
    h.synchronize()
    others = np.arange(len(pos)) != row
    for k in _lib.TRANSPORT_OUTPUTS:
        a, b = clean[k].cpu().numpy(), dirty[k].cpu().numpy()
        assert a[others].tobytes() == b[others].tobytes(), k
        print(k, "NaN row:", b[row])
        if not k.startswith("post_"):
            assert np.all(np.isnan(b[row])), k
    # post_*: what the library's own posterior launches give for that query, which is theirs to define (the mean kernel returns
    # the prior mean, 0, for a NaN query); the epilogue's own outputs above are NaN whatever it read there
    M = len(pos)
    mean, J, Jvar = (torch.empty_like(dirty[k]) for k in ("post_mean", "post_J", "post_Jvar"))
    var, J_ori = torch.empty_like(dirty["var"]), torch.empty_like(dirty["post_J_ori"])
    h.predict_all_dev(dirty["pos_rot"].data_ptr(), M, mean.data_ptr(), var.data_ptr(), J.data_ptr(), Jvar.data_ptr())
    h.predict_all_dev(keep2["pos"].data_ptr(), M, 0, 0, J_ori.data_ptr())
    h.synchronize()
    for k, t in (("post_mean", mean), ("var", var), ("post_J", J), ("post_Jvar", Jvar), ("post_J_ori", J_ori)):
        assert dirty[k].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), k
