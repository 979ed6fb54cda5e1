"""The inverse of the transport map: AffineTransform.inverse_predict, GaussianProcess.invert_displacement (damped Newton on the
device, one wave per query, one launch: csrc/gpt_inverse.hip), PolicyTransportation.inverse_transport.

The reference has no inverse to match (its inverse-mapping example fits a second transport backwards), so the anchors are its
FORWARD goldens read the other way — the reference's outputs, inverted, must give the reference's inputs — and the numpy
restatement of the iteration in tests/inverse_map_restatement.py.

Bounds.  A CONVERGED z satisfies |z + mu(z) - y| <= rtol (1 + |y|) up to the rounding floor of the device's sums, 64 eps S
(S: norm over the outputs of sum_n |k(z, X_n) alpha_n|), so it is within (rtol (1 + |y|) + floor) |A^-1|_2 of the exact preimage
to first order, A = I + J(z); the tests allow twice that (inverse_map_restatement.error_bound).

Not tested: SINGULAR in 1-D.  With D = 1 the criterion |det A| <= 2^-40 |A|_F^D reads |A| <= 2^-40 |A|, which
holds only for A == 0 exactly, and no start point can be placed so that the device's own sum rounds to exactly -1.  The same
construction in 2-D (below) can be placed: there |A|_F stays ~1 while det passes through zero."""
import numpy as np
import pytest

from tests import inverse_map_restatement as R
from tests.conftest import load_golden, relmax

EPS = np.finfo(np.float64).eps
RTOL = 1e-10


def sk_rbf(c, ls, noise):
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    return ConstantKernel(float(c)) * RBF(length_scale=np.atleast_1d(np.asarray(ls, dtype=float)).tolist()) + WhiteKernel(float(noise))


def sk_matern(c, ls, nu, noise):
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel
    return ConstantKernel(c) * Matern(length_scale=ls, nu=nu) + WhiteKernel(noise)


def _transport_case(name):
    """Golden fixture, the oracle's affine part and GP at the golden theta, and the restatement's model of it."""
    from oracle.gp_oracle import AffineTransformOracle, GaussianProcessOracle
    g = load_golden(name)
    aff = AffineTransformOracle().fit(g["source"], g["target"])
    src = aff.predict(g["source"])
    gp = GaussianProcessOracle(g["constant_value"], g["length_scale"], g["noise_level"]).fit(src, g["target"] - src)
    return {"g": g, "aff": aff, "model": R.RbfModel(gp), "pos": aff.predict(g["demo"])}


@pytest.fixture(scope="module")
def letter():
    return _transport_case("letterS_2d")


@pytest.fixture(scope="module")
def surface():
    return _transport_case("surface_3d")


def _counts(info):
    return np.bincount(info["status"], minlength=4)


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ["letterS_2d", "surface_3d"])
@pytest.mark.parametrize("do_scale", [False, True])
def test_affine_inverse_predict(name, do_scale):
    from gaussian_process_transportation_amd.affine_transform import AffineTransform
    g = load_golden(name)
    aff = AffineTransform(do_scale=do_scale, verbose=False).fit(g["source"], g["target"])
    if do_scale:
        assert aff.scale != 1
    for x in (g["demo"], g["source"]):
        assert relmax(aff.inverse_predict(aff.predict(x)), x) <= 1e-13


def test_surface_anchor_restatement(surface):
    """The reference's transported trajectory, pulled back, is the (aligned) demonstration it was made from."""
    y = surface["g"]["traj"]
    z, info = R.inverse_map(surface["model"], y, rtol=RTOL)
    print("surface_3d restatement: status", _counts(info), "passes", info["passes"].min(), "..", info["passes"].max())
    assert np.all(info["status"] == R.CONVERGED)
    assert info["passes"].max() <= 8
    bound, _ = R.error_bound(surface["model"], z, y, RTOL)
    err = np.linalg.norm(z - surface["pos"], axis=1)
    print(f"surface_3d restatement: error max {err.max():.2e}, largest share of the bound {np.max(err / bound):.2f}")
    assert np.all(err <= 2 * bound)


def test_letterS_baseline_restatement(letter):
    """The numbers the GPU test leans on: the reference's letter-S map folds (21 of its 400 forward determinants are not
    positive), and the restatement still solves all but a few of the 400 golden points."""
    pos, y = letter["pos"], letter["g"]["traj"]
    det_fwd = np.linalg.det(R.residual_and_jacobian(letter["model"], pos, pos)[1])
    assert int(np.sum(det_fwd <= 0)) == 21
    z, info = R.inverse_map(letter["model"], y, rtol=RTOL)
    ok = info["status"] == R.CONVERGED
    print("letterS restatement: status", _counts(info), "passes", info["passes"].min(), "..", info["passes"].max(),
          f"residual of the converged <= {info['residual'][ok].max():.1e}, det <= 0 at {int(np.sum(info['det'][ok] <= 0))} solutions")
    assert int(np.sum(~ok)) <= 4
    assert np.all(info["residual"][ok] <= RTOL * (1 + np.linalg.norm(y[ok], axis=1)))
    assert int(np.sum(info["det"][ok] <= 0)) > 0
    assert info["passes"].max() > 8             # (the launch the GPU test makes holds queries of very different lengths)


@pytest.mark.parametrize("name", ["synthetic_3d_N64", "synthetic_3d_N256"])
def test_synthetic_restatement(name):
    from oracle.gp_oracle import GaussianProcessOracle
    g = load_golden(name)
    gp = GaussianProcessOracle(g["constant_value"], g["length_scale"], g["noise_level"], float(g["alpha"])).fit(g["X"], g["Y"])
    model = R.RbfModel(gp)
    y = g["Xq"] + gp.predict(g["Xq"])
    z, info = R.inverse_map(model, y, rtol=RTOL)
    assert np.all(info["status"] == R.CONVERGED) and info["passes"].max() <= 7 and info["det"].min() >= 0.36
    assert np.all(np.linalg.norm(z - g["Xq"], axis=1) <= 2 * R.error_bound(model, z, y, RTOL)[0])


class OraclePlugin:
    """A delta_map for PolicyTransportation on the CPU oracle, with invert_displacement through the restatement."""

    def __init__(self, c, ls, noise):
        from oracle.gp_oracle import GaussianProcessOracle
        self.gp = GaussianProcessOracle(c, ls, noise)

    def fit(self, X, Y):
        self.gp.fit(X, Y)

    def predict(self, x, return_std=False):
        return self.gp.predict(x, return_std=return_std)

    def invert_displacement(self, y, x0=None, rtol=1e-10, max_passes=64, return_info=False):
        z, info = R.inverse_map(R.RbfModel(self.gp), y, x0, rtol=rtol, max_passes=max_passes)
        return (z, info) if return_info else z


def test_policy_inverse_transport_host_algebra(letter, capsys):
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    from gaussian_process_transportation_amd.policy_transportation import PolicyTransportation
    g = letter["g"]
    for do_scale in (False, True):
        pt = PolicyTransportation(OraclePlugin(g["constant_value"], g["length_scale"], g["noise_level"]), verbose=False)
        pt.fit(g["source"], g["target"], do_scale=do_scale)
        fwd = pt.transport(g["demo"], return_std=False)[0]
        x, info = pt.inverse_transport(fwd, return_info=True)
        ok = info["status"] == R.CONVERGED
        assert int(np.sum(~ok)) <= 4
        back = pt.transport(x, return_std=False)[0]                       # Phi(Phi^-1(y)) = y, whichever preimage was found
        assert np.all(np.linalg.norm(back - fwd, axis=1)[ok] <= 2 * RTOL * (1 + np.linalg.norm(fwd, axis=1)[ok]))
        x1, info1 = pt.inverse_transport(fwd, x0=g["demo"], return_info=True)       # started at the preimage: nothing to do
        assert np.all(info1["passes"] == 1) and np.all(info1["status"] == R.CONVERGED)
        assert relmax(x1, g["demo"]) <= 1e-13
        assert pt.inverse_transport(fwd, max_passes=2).shape == fwd.shape           # solver arguments reach the delta_map
        assert np.any(pt.inverse_transport(fwd, max_passes=2, return_info=True)[1]["status"] == R.MAX_PASSES)
    capsys.readouterr()
    pt.verbose = True
    pt.inverse_transport(fwd)
    said = capsys.readouterr().out
    assert "CONVERGED" in said and "STALLED" in said and "det(I + J_psi) <= 0" in said

    class NoInverse:
        def fit(self, X, Y): pass
    bare = PolicyTransportation(NoInverse(), verbose=False)
    bare.fit(g["source"], g["target"])
    with pytest.raises(NotImplementedError, match="invert_displacement"):
        bare.inverse_transport(fwd)
    tr = GaussianProcessTransportation(optimizer=None, verbose=False)             # the user-facing class delegates
    tr.method = pt
    pt.verbose = False
    assert np.array_equal(tr.inverse_transport(fwd, x0=g["demo"]), x1)


# ------------------------------------------------------------------------------------------------------------ GPU
def _fit_transport(g, **kw):
    from gaussian_process_transportation_amd import GaussianProcessTransportation
    tr = GaussianProcessTransportation(kernel_transport=sk_rbf(g["constant_value"], g["length_scale"], g["noise_level"]),
                                       optimizer=None, verbose=False, **kw)
    tr.source_distribution, tr.target_distribution = g["source"], g["target"]
    tr.fit_transportation()
    return tr


@pytest.fixture(scope="module")
def letter_gpu(letter):
    """The letter-S transport on the device and its inverse at the 400 golden points (cases 2, 3, 5 share it)."""
    tr = _fit_transport(letter["g"])
    gp = tr.method.delta_map
    z, info = gp.invert_displacement(letter["g"]["traj"], rtol=RTOL, return_info=True)
    return {"tr": tr, "gp": gp, "z": z, "info": info}


def _forward_residual(gp, z, y):
    return np.linalg.norm(z + gp.predict(z) - y, axis=1)


def _floor(model, z):
    return 64 * EPS * np.linalg.norm(model.abs_sum(z), axis=1)


@pytest.mark.gpu
def test_surface_3d_inverse_gives_the_demonstration(surface):
    g = surface["g"]
    tr = _fit_transport(g)
    x, info = tr.inverse_transport(g["traj"], return_info=True, rtol=RTOL)
    print("surface_3d: status", _counts(info), "passes", info["passes"].min(), "..", info["passes"].max())
    assert np.all(info["status"] == R.CONVERGED)
    z = surface["aff"].predict(x)
    bound, _ = R.error_bound(surface["model"], z, g["traj"], RTOL)
    err = np.linalg.norm(x - g["demo"], axis=1)
    print(f"surface_3d: error max {err.max():.2e}, largest share of the bound {np.max(err / bound):.2f}")
    assert np.all(err <= 2 * bound)


@pytest.mark.gpu
def test_letterS_inverse_reports_the_fold(letter, letter_gpu):
    y, gp, z, info = letter["g"]["traj"], letter_gpu["gp"], letter_gpu["z"], letter_gpu["info"]
    ok = info["status"] == R.CONVERGED
    print("letterS: status", _counts(info), "passes", info["passes"].min(), "..", info["passes"].max())
    assert int(np.sum(~ok)) <= 4
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(info["residual"])) and np.all(np.isfinite(info["det"]))
    res = _forward_residual(gp, z, y)
    floor = _floor(letter["model"], z)
    print(f"letterS: recomputed residual of the converged <= {res[ok].max():.2e}; floor <= {floor.max():.1e}")
    assert np.all(res[ok] <= RTOL * (1 + np.linalg.norm(y[ok], axis=1)) + floor[ok])
    det = np.linalg.det(np.eye(2)[None] + gp.derivative(z))
    assert np.all(np.abs(info["det"] - det) <= 1e-9)
    assert int(np.sum(info["det"][ok] <= 0)) > 0
    # a query that did not converge reports the residual it reached (both sides carry the rounding of their own sums)
    assert np.all(np.abs(info["residual"] - res) <= 2 * floor + 8 * EPS * (1 + np.linalg.norm(y, axis=1)))


@pytest.mark.gpu
def test_query_independence_bitwise(letter, letter_gpu):
    y, h = letter["g"]["traj"], letter_gpu["gp"]._handle
    for k in (1, 5, 64, 65):                          # 1 and 5: workgroups whose four waves are not all used
        z, info = h.inverse_map(y[:k], rtol=RTOL)
        assert z.tobytes() == letter_gpu["z"][:k].tobytes(), k
        for key in ("status", "passes", "residual", "det"):
            assert info[key].tobytes() == letter_gpu["info"][key][:k].tobytes(), (k, key)


def _synthetic_gp(kind):
    from gaussian_process_transportation_amd import GaussianProcess
    from oracle.gp_oracle import GaussianProcessOracle
    g = load_golden("synthetic_3d_N256" if kind == "rbf256" else "synthetic_3d_N64")
    if kind.startswith("rbf"):
        gp = GaussianProcess(kernel=sk_rbf(g["constant_value"], g["length_scale"], g["noise_level"]), alpha=float(g["alpha"]),
                             optimizer=None, verbose=False).fit(g["X"], g["Y"])
        orc = GaussianProcessOracle(g["constant_value"], g["length_scale"], g["noise_level"], float(g["alpha"])).fit(g["X"], g["Y"])
        return g, gp, R.RbfModel(orc)
    nu, c, ls, noise = float(kind[6:]), 0.1, np.array([0.3, 0.25, 0.35]), 1e-4
    gp = GaussianProcess(kernel=sk_matern(c, ls, nu, noise), optimizer=None, verbose=False, matern_derivatives=True).fit(g["X"], g["Y"])
    return g, gp, R.MaternModel(g["X"], g["Y"], c, ls, nu, noise)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rbf64", "rbf256", "matern1.5", "matern2.5"])
def test_synthetic_round_trip(kind):
    g, gp, model = _synthetic_gp(kind)
    Xq = g["Xq"]
    y = Xq + gp.predict(Xq)
    z, info = gp.invert_displacement(y, rtol=RTOL, return_info=True)
    print(kind, "status", _counts(info), "passes <=", info["passes"].max(), "det >=", info["det"].min())
    assert np.all(info["status"] == R.CONVERGED)
    err = np.linalg.norm(z - Xq, axis=1)
    bound, _ = R.error_bound(model, z, y, RTOL)
    print(f"{kind}: error max {err.max():.2e}, largest share of the bound {np.max(err / bound):.2f}")
    assert np.all(err <= 2 * bound)


@pytest.mark.gpu
def test_start_point_and_pass_limits(letter, letter_gpu):
    gp, pos, y = letter_gpu["gp"], letter["pos"], letter["g"]["traj"]
    # started at the preimage: one pass, the start comes back unchanged
    y_own = pos + gp.predict(pos)
    z, info = gp.invert_displacement(y_own, x0=pos, rtol=RTOL, return_info=True)
    assert np.all(info["passes"] == 1) and np.all(info["status"] == R.CONVERGED) and z.tobytes() == pos.tobytes()
    # one pass allowed: the residual at the start decides, nothing moves
    z, info = gp.invert_displacement(y, rtol=RTOL, max_passes=1, return_info=True)
    tol = RTOL * (1 + np.linalg.norm(y, axis=1))
    assert np.all(info["passes"] == 1) and z.tobytes() == np.ascontiguousarray(y).tobytes()
    assert np.array_equal(info["status"], np.where(info["residual"] > tol, R.MAX_PASSES, R.CONVERGED))
    assert np.any(info["status"] == R.MAX_PASSES)
    # three passes: some queries are done, the others report where they stand
    z, info = gp.invert_displacement(y, rtol=RTOL, max_passes=3, return_info=True)
    n = _counts(info)
    print("letterS, max_passes = 3: status", n)
    assert n[R.CONVERGED] > 0 and n[R.MAX_PASSES] > 0 and n[R.CONVERGED] + n[R.MAX_PASSES] == len(y)
    assert np.all(info["passes"][info["status"] == R.MAX_PASSES] == 3)
    res = _forward_residual(gp, z, y)
    assert np.all(np.abs(info["residual"] - res) <= 2 * _floor(letter["model"], z) + 8 * EPS * (1 + np.linalg.norm(y, axis=1)))
    assert np.all((info["residual"] <= tol) == (info["status"] == R.CONVERGED))


@pytest.mark.gpu
def test_singular_start_is_reported():
    """A start point where I + J is singular, found without provoking anything: psi_1(x) ~ -x_1 on a grid, psi_2 = 0, so that
    det(I + J) = 1 + d psi_1 / d x_1 passes through zero along x_1 while |I + J|_F stays 1.  The restatement bisects the
    crossing to the last bit of x_1; there |det| ~ 1e-16 on the CPU and, with sum_n |dk alpha| = 18, within 64 eps 18 = 2.6e-13 of
    that on the device at worst — inside the 2^-40 |A|_F^2 = 9.1e-13 of the criterion."""
    from gaussian_process_transportation_amd import GaussianProcess
    from oracle.gp_oracle import GaussianProcessOracle
    gx = np.linspace(0, 1, 10)
    X = np.stack(np.meshgrid(gx, gx, indexing="ij"), -1).reshape(-1, 2)
    Y = np.stack([-X[:, 0], np.zeros(len(X))], axis=1)
    c, ls, noise = 1.0, [0.7, 0.7], 1e-2
    model = R.RbfModel(GaussianProcessOracle(c, ls, noise).fit(X, Y))

    def det_at(x1):
        z = np.array([[x1, 0.5]])
        return np.linalg.det(R.residual_and_jacobian(model, z, z)[1])[0]
    a, b = 0.3, 0.6
    assert det_at(a) > 0 > det_at(b)
    while True:
        mid = 0.5 * (a + b)
        if mid == a or mid == b:
            break
        a, b = (mid, b) if det_at(mid) > 0 else (a, mid)
    x1 = a if abs(det_at(a)) <= abs(det_at(b)) else b
    z0 = np.array([[x1, 0.5]])
    A = R.residual_and_jacobian(model, z0, z0)[1][0]
    assert abs(np.linalg.det(A)) <= 1e-14 and np.sum(A * A) >= 1.0           # the start is placed; the criterion has room
    gp = GaussianProcess(kernel=sk_rbf(c, ls, noise), optimizer=None, verbose=False).fit(X, Y)
    y = z0 + gp.predict(z0) + np.array([[0.05, 0.0]])
    z, info = gp.invert_displacement(y, x0=z0, return_info=True)
    assert info["status"][0] == R.SINGULAR and info["passes"][0] == 1
    assert z.tobytes() == z0.tobytes() and abs(info["det"][0]) <= 2.0 ** -40 * np.sum(A * A) and np.isfinite(info["residual"][0])
    assert info["residual"][0] == pytest.approx(0.05, rel=1e-9)


@pytest.mark.gpu
def test_refusals():
    from gaussian_process_transportation_amd import GaussianProcess, _lib
    rng = np.random.default_rng(0)
    X3 = rng.uniform(0, 1, (50, 3)); q3 = rng.uniform(0, 1, (4, 3))
    gp = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False)
    with pytest.raises(RuntimeError, match="not fitted"):
        gp.invert_displacement(q3)
    h = _lib.Handle(0)
    with pytest.raises(_lib.GptError, match="not fitted"):                     # GPT_E_STATE
        h.inverse_map(q3)
    gp.fit(X3, 0.05 * np.sin(4 * X3))
    z, info = gp.invert_displacement(np.zeros((0, 3)), return_info=True)        # M = 0: nothing to do
    assert z.shape == (0, 3) and info["status"].shape == (0,)
    for bad, match in ((dict(rtol=0.0), "rtol"), (dict(rtol=-1e-3), "rtol"), (dict(rtol=float("nan")), "rtol"), (dict(max_passes=0), "max_passes")):
        with pytest.raises(ValueError, match=match):
            gp.invert_displacement(q3, **bad)
        with pytest.raises(ValueError, match=match):                           # GPT_E_ARG from the library itself
            gp._handle.inverse_map(q3, **bad)
    for y, x0 in ((np.full((4, 3), np.nan), None), (q3, np.full((4, 3), np.inf))):
        with pytest.raises(ValueError, match="NaN or infinity"):
            gp.invert_displacement(y, x0=x0)
    for y, x0 in ((np.full((4, 3), np.nan), None), (q3, np.full((4, 3), np.inf))):      # the C entry point checks for itself
        zz = np.empty((4, 3)); st = np.empty(4, dtype=np.int32)
        rc = h.lib.gpt_inverse_map(gp._handle._h, _lib.dptr(np.ascontiguousarray(y)), _lib.dptr(x0), 4, 1e-10, 64, _lib.dptr(zz), None, None,
                                   None, st.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int)))
        assert rc == _lib.GPT_E_ARG and "NaN or infinity" in _lib.last_error()
    rc = h.lib.gpt_inverse_map_dev(gp._handle._h, None, None, -1, 1e-10, 64, None, None, None, None, None)
    assert rc == _lib.GPT_E_ARG and "2^31" in _lib.last_error()
    rc = h.lib.gpt_inverse_map_dev(gp._handle._h, None, None, 2 ** 31, 1e-10, 64, None, None, None, None, None)
    assert rc == _lib.GPT_E_ARG and "2^31" in _lib.last_error()
    with pytest.raises(ValueError, match="columns"):
        gp.invert_displacement(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="shape"):
        gp.invert_displacement(q3, x0=q3[:2])
    # D != O, D > 3
    two_out = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False).fit(X3, X3[:, :2])
    with pytest.raises(NotImplementedError, match="onto itself"):
        two_out.invert_displacement(q3)
    with pytest.raises(ValueError, match="D == O"):
        two_out._handle.inverse_map(q3)
    X4 = rng.uniform(0, 1, (50, 4))
    wide = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False).fit(X4, 0.05 * np.sin(X4))
    with pytest.raises(NotImplementedError, match="at most 3"):
        wide.invert_displacement(X4[:3])
    with pytest.raises(ValueError, match="D <= 3"):
        wide._handle.inverse_map(X4[:3])
    # fp32 and multi-task models
    f32 = GaussianProcess(kernel=sk_rbf(0.1, [0.3], 1e-3), optimizer=None, verbose=False, dtype="float32").fit(X3, 0.05 * np.sin(X3))
    with pytest.raises(NotImplementedError, match="float64"):
        f32.invert_displacement(q3)
    with pytest.raises(ValueError, match="fp64"):
        f32._handle.inverse_map(q3)
    h.fit_svgp(X3, rng.standard_normal((3, 50)), 1e-2 * np.eye(50) * np.ones((3, 1, 1)), np.full(3, 0.3), np.ones(3))
    with pytest.raises(ValueError, match="single-task"):
        h.inverse_map(q3)
    h.close()
    # Matern: 1/2 never, 3/2 and 5/2 only with the analytic derivatives enabled
    m12 = GaussianProcess(kernel=sk_matern(0.1, 0.3, 0.5, 1e-3), optimizer=None, verbose=False, matern_derivatives=True).fit(X3, 0.05 * np.sin(X3))
    with pytest.raises(NotImplementedError, match="nu=0.5"):
        m12.invert_displacement(q3)
    with pytest.raises(ValueError, match="Matern 1/2"):
        m12._handle.inverse_map(q3)
    m52 = GaussianProcess(kernel=sk_matern(0.1, 0.3, 2.5, 1e-3), optimizer=None, verbose=False).fit(X3, 0.05 * np.sin(X3))
    with pytest.raises(NotImplementedError, match="matern_derivatives"):
        m52.invert_displacement(q3)
    with pytest.raises(ValueError, match="gpt_set_matern_derivatives"):
        m52._handle.inverse_map(q3)


@pytest.mark.gpu
def test_device_pointer_entry_on_a_callers_stream(letter, letter_gpu):
    import torch
    y, gp, h = letter["g"]["traj"], letter_gpu["gp"], letter_gpu["gp"]._handle
    before = h.predict_all(letter["pos"], mean=True, var=True, J=True, Jvar=True)
    dev = torch.device("cuda", 0)
    M = len(y)
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
    z = torch.empty((M, 2), dtype=torch.float64, device=dev)
    res = torch.empty(M, dtype=torch.float64, device=dev); det = torch.empty(M, dtype=torch.float64, device=dev)
    npass = torch.empty(M, dtype=torch.int32, device=dev); status = torch.empty(M, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    h.set_stream(stream.cuda_stream)
    try:
        h.inverse_map_dev(yd.data_ptr(), M, z.data_ptr(), status.data_ptr(), residual_ptr=res.data_ptr(), det_ptr=det.data_ptr(),
                          passes_ptr=npass.data_ptr(), rtol=RTOL)
        stream.synchronize()
        z2 = torch.empty_like(z); st2 = torch.empty_like(status)
        h.inverse_map_dev(yd.data_ptr(), M, z2.data_ptr(), st2.data_ptr(), rtol=RTOL)      # the optional outputs left out
        stream.synchronize()
    finally:
        h.set_stream(0)
    assert z.cpu().numpy().tobytes() == letter_gpu["z"].tobytes() and z2.cpu().numpy().tobytes() == letter_gpu["z"].tobytes()
    for key, t in (("status", status), ("status", st2), ("passes", npass), ("residual", res), ("det", det)):
        assert t.cpu().numpy().tobytes() == letter_gpu["info"][key].tobytes(), key
    after = h.predict_all(letter["pos"], mean=True, var=True, J=True, Jvar=True)        # the model and its scratch are untouched
    for key in before:
        if before[key] is not None:
            assert before[key].tobytes() == after[key].tobytes(), key
