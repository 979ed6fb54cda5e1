"""Paths of functions drawn from the dynamics posterior in one device call: gpt_rollout_sampled (csrc/gpt_rollout_sampled.hip:
sixteen paths per workgroup, u = W k* on the matrix cores, the growing Cholesky factor of a path's covariance inside the step
loop), GaussianProcess.rollout_samples / rollout_chain_samples, TransportChain.rollout_samples and the transport classes'
rollout_policy_samples.

What holds the kernel:
  1. zero normals are the merged mean rollout, bit for bit (every line of the new body but the draw's own).
  2. step-local correctness at the device's OWN points (the dynamics amplifies rounding, so nothing is compared end to end):
     G G^T against the path's posterior covariance recomputed in longdouble from the returned x, within
     (1024 + 4 (T + 1)) ulps of c + nugget: the bound tests/test_input_ranges.py holds variances to (MARGIN x FLOOR_ULPS,
     rollout_stab_restatement.PAIR_TOL) plus the backward error of a Cholesky factor of T rows; pvar against the merged variance
     launch (PAIR_TOL); cvar = diag(G)^2; vel from the device's own f and G; path by euler_step of the device's vel, exactly;
     f bitwise the mean rollout's.
  3. the edges of the sweep (N), of a factor row's register chunks (T) and of the tile's columns (P).
  4. independence of P, neighbours, order, column, launch cuts and host chunks, bit for bit.
  5. the degenerate end.  6. refusals."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import posterior_restatement as PR
from tests import rollout_sampled_restatement as SR
from tests import rollout_stab_restatement as RS
from tests.conftest import load_golden
from tests.test_policy_rollout import M9, T12, _letter_starts, _sentinels, _stage_tuples
from tests.test_pullback_policy import EPS, LD, RTOL, SENT, _fit_gp, _untouched
from tests.test_rollout_stabilised import _fold_starts, _mean, _pushed, _recorded, letter2, surface3      # noqa: F401 (fixtures)

MEAN_NAMES = ("path", "vel", "x", "steps_done", "status")
ALL_NAMES = ("path", "vel", "x", "f", "pvar", "cvar", "chol", "steps_done", "status")
NU = {"rbf": None, "matern12": 0.5, "matern32": 1.5, "matern52": 2.5}
CHOL_ULPS = lambda T: PR.MARGIN * PR.FLOOR_ULPS + 4 * (T + 1)


# ------------------------------------------------------------------------------------------------------------ helpers
def _samp(chain, dyn, y0, normals, nugget=None, dt=1.0, x0=None, **solver):
    """The device call through the public interface, one sample per start: every array with the leading shape (P,)."""
    y0, normals = np.ascontiguousarray(y0), np.ascontiguousarray(normals)
    T = normals.shape[1]
    if chain is None:
        path, info = dyn.rollout_samples(y0, T, n_samples=1, dt=dt, nugget=nugget, normals=normals[:, None], return_info="chol")
    else:
        path, info = chain.rollout_samples(dyn, y0, T, n_samples=1, dt=dt, nugget=nugget, normals=normals[:, None], x0=x0, return_info="chol", **solver)
    return {k: v[:, 0] for k, v in dict(info, path=path).items()}


def _normals(P, T, D, seed=0):
    return np.random.RandomState(seed).standard_normal((P, T, D))


def _same(got, want, what, names=ALL_NAMES):
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def _same_path(got, i, want, j, what):
    for k in ALL_NAMES:
        assert_array_equal(got[k][i], want[k][j], err_msg=f"{what}: {k}")


def _check_nan_layout(out):
    """tests/test_rollout_stabilised.py::_check_nan_layout in this call's names: everything after a path's end is NaN; what the
    last step evaluated (x, f, pvar, and cvar unless it is the NaN that ended the path) is there."""
    T = out["vel"].shape[1]
    for m, done in enumerate(out["steps_done"]):
        last = min(int(done) + 1, T)
        assert np.all(np.isfinite(out["path"][m, :done + 1])) and np.all(np.isnan(out["path"][m, done + 1:])), m
        for k in ("vel", "x", "f", "pvar", "cvar", "chol"):
            assert np.all(np.isnan(out[k][m, last:])), (k, m)
        for k in ("x", "f", "pvar"):
            assert np.all(np.isfinite(out[k][m, :last])), (k, m)
        assert np.all(np.isfinite(out["vel"][m, :done])) and np.all(np.isfinite(out["chol"][m, :done])) and np.all(np.isfinite(out["cvar"][m, :done]))
        if out["status"][m] == SR.DEGENERATE:
            assert done < T and np.all(np.isnan(out["vel"][m, done])) and np.all(np.isnan(out["chol"][m, done]))


_LD_MODELS = {}


def _ld_model(gp, kind):
    key = (id(gp), kind)
    if key not in _LD_MODELS:
        _LD_MODELS[key] = (gp, SR.Model(gp.X, gp.Y if hasattr(gp, "Y") else np.zeros((len(gp.X), 1)), gp._c, gp._ls, gp._noise, gp.alpha, kind, LD))
    return _LD_MODELS[key][1]


def _check_factor(out, gp, kind, nugget, what, paths=None, cov_of=None):
    """Check 2, the factor: per path, G G^T against the covariance of the device's own points.  cov_of(x (t,D)) -> (t,t) overrides
    the longdouble restatement (N > LML_CHECK_MAX_N); the bound is then the caller's."""
    T = out["vel"].shape[1]
    scale = gp._c + nugget
    worst = 0.0
    for p in (range(len(out["steps_done"])) if paths is None else paths):
        t = int(out["steps_done"][p])
        if t == 0:
            continue
        G = out["chol"][p, :t, :t]
        assert np.all(np.triu(G, 1) == 0) and np.all(np.diag(G) > 0) and np.all(out["chol"][p, :t, t:] == 0), (what, p)
        x = out["x"][p, :t]
        if cov_of is None:
            C = SR.path_terms(_ld_model(gp, kind), x, nugget)["cov"]
            ulps = CHOL_ULPS(T)
        else:
            C, ulps = cov_of(x)
        err = np.abs((G.astype(LD) @ G.T.astype(LD)) - C).astype(np.float64)
        worst = max(worst, float(err.max()) / (ulps * EPS * scale))
        assert np.all(err <= ulps * EPS * scale), (what, p, float(err.max()) / (EPS * scale), ulps)
        # cvar is the squared diagonal, to 2 ulps
        cv = out["cvar"][p, :t]
        assert np.all(np.abs(np.diag(G) ** 2 - cv) <= 2 * EPS * cv), (what, p)
    print(f"{what}: |G G^T - C| largest share of the bound {worst:.4f}")


def _check_pvar(out, gp, nugget, what):
    """pvar of every recorded step against the merged variance launch at the device's x_t: both are c + (diagonal) - |W k*|^2."""
    rec = _recorded(out)
    xq = np.ascontiguousarray(np.stack([out["x"][m, t] for m, t in rec]))
    ref = gp._handle.predict_all(xq, var=True)["var"].reshape(-1)
    pv = np.array([out["pvar"][m, t] for m, t in rec])
    e = np.abs((pv - nugget) - (ref - gp._noise)) / (gp._c + max(nugget, gp._noise))
    print(f"{what}: {len(rec)} steps; pvar against the merged launch {float(e.max()) / RS.PAIR_TOL:.4f} of the bound")
    assert np.all(e <= RS.PAIR_TOL), what


def _check_velocity(out, normals, dt, what, chain=None, dyn=None, **solver):
    """vel from the device's own f and G, and the Euler step.  K = 0: within (t + 3) ulps of |f| + sum |g z| (t + 1 products and
    sums, each rounded once, and the sum with f).  K >= 1: the draw pushed through the maps as tests/test_rollout_stabilised.py
    pushes fs, with its 4 ulps of the push added: ((t + 3) + 4) ulps of the largest |f_d| + sum |g z_d| times the 1-norm of the
    matrix applied."""
    worst = 0.0
    for m, t in _recorded(out):
        if t < out["steps_done"][m]:
            assert_array_equal(out["path"][m, t + 1], out["path"][m, t] + dt * out["vel"][m, t], err_msg=f"{what} step {m},{t}")
        g = out["chol"][m, t, :t + 1]
        if not np.all(np.isfinite(g)):
            continue
        f, z = out["f"][m, t], normals[m, :t + 1]
        fs = (f.astype(LD) + (g.astype(LD)[:, None] * z.astype(LD)).sum(0)).astype(np.float64)
        mag = np.abs(f) + (np.abs(g)[:, None] * np.abs(z)).sum(0)
        if chain is None:
            want, tol = fs, (t + 3) * EPS * mag
        else:
            want, norm = _pushed(chain, dyn, out, m, t, fs, solver)
            tol = (t + 3 + 4) * EPS * np.max(mag) * norm
        err = np.abs(out["vel"][m, t] - want)
        worst = max(worst, float(np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(err <= tol), (what, m, t, out["vel"][m, t], want, tol)
    print(f"{what}: vel against the definition from the device's f and chol: largest share of the bound {worst:.3f}")


@pytest.fixture(scope="module")
def letter_kernels():
    """The letter-S dynamics (400 points) with each of the four kernels."""
    g = load_golden("letterS_2d")
    return {kind: _fit_gp(g["demo"], g["delta"], 0.3, [1.5, 2.5], 0.01, nu) for kind, nu in NU.items()}, g


# ------------------------------------------------------------------------------------------------------------ 1. zero normals
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["K=0 3-D", "K=2 2-D"])
def test_zero_normals_are_the_mean_rollout(which, letter2, surface3):
    if which == "K=0 3-D":
        chain, dyn, y0, X, solver = None, surface3["dyn"], surface3["X"], None, {}
    else:
        chain, dyn, solver = letter2["chain"], letter2["gp_dyn"], dict(rtol=RTOL)
        y0, X = _letter_starts(letter2["g"])
    for dt in (0.5, -1.0):
        got = _samp(chain, dyn, y0, np.zeros((M9, T12, y0.shape[1])), dt=dt, x0=X, **solver)
        want = _mean(chain, dyn, y0, T12, dt=dt, x0=X, **solver)
        for k in MEAN_NAMES:                                     # (== : +0 and -0 agree; NaN positions the same)
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype
            assert np.all((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))), (which, dt, k)
        assert np.any(got["steps_done"] == T12)
        _check_nan_layout(got)


# ------------------------------------------------------------------------------------------------------------ 2. step-local
@pytest.mark.gpu
@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("nugget", ["noise", 1e-6])
def test_step_local(kind, nugget, letter_kernels):
    gps, g = letter_kernels
    gp = gps[kind]
    nugget = gp._noise if nugget == "noise" else nugget
    P, T, dt = 5, T12, 1.0
    y0 = np.ascontiguousarray(g["demo"][::90][:P] + 0.01)
    z = _normals(P, T, 2, 3)
    out = _samp(None, gp, y0, z, nugget=nugget, dt=dt)
    what = f"{kind}, nugget {nugget:g}"
    assert np.all(out["steps_done"] == T) and np.all(out["status"] == SR.CONVERGED), what
    _check_nan_layout(out)
    _check_factor(out, gp, kind, nugget, what)
    _check_pvar(out, gp, nugget, what)
    _check_velocity(out, z, dt, what)
    # f_t is the mean rollout's velocity at x_t, bitwise; x_t is the path's point
    xs = np.ascontiguousarray(out["x"].reshape(-1, 2))
    assert_array_equal(gp.rollout(xs, 1, return_info=True)[1]["vel"][:, 0], out["f"].reshape(-1, 2))
    assert_array_equal(out["x"], out["path"][:, :T])
    # the draw does something
    assert not np.array_equal(out["path"], gp.rollout(y0, T, dt=dt))


@pytest.mark.gpu
def test_step_local_through_two_maps(letter2):
    chain, dyn = letter2["chain"], letter2["gp_dyn"]
    y0, X = _letter_starts(letter2["g"])
    z = _normals(M9, T12, 2, 4)
    for nugget in (None, 1e-6):
        out = _samp(chain, dyn, y0, z, nugget=nugget, dt=0.5, x0=X, rtol=RTOL)
        nug = dyn._noise if nugget is None else nugget
        assert np.any(out["steps_done"] == T12)
        _check_nan_layout(out)
        _check_factor(out, dyn, "rbf", nug, f"K = 2, nugget {nug:g}")
        _check_pvar(out, dyn, nug, "K = 2")
        _check_velocity(out, z, 0.5, "K = 2", chain=chain, dyn=dyn, x0_first=X, rtol=RTOL)


# ------------------------------------------------------------------------------------------------------------ 3. edges
def _synthetic(N, D, kind, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    ls = np.array([0.2, 0.3, 0.25])[:D] * (1.0 if D > 1 else 0.25)
    return _fit_gp(X, 0.1 * (np.cos(3 * X) - 0.5), 0.5, ls, 1e-3, NU[kind]), rng


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 511, 512, 513, 1024])
def test_sweep_edges(N):
    """The sizes where the sweep changes shape (a row group, a 512-tile of the packed factor, two); T = 5, P = 5, the four
    kernels over D = 1, 2, 3.  Beyond LML_CHECK_MAX_N points the covariance reference is the merged predict(return_cov=True)
    launch at the device's points, diagonal moved from the noise to the nugget, and the bound the sum of both launches' (1024 ulps
    each) plus the Cholesky term."""
    for D, kind in ((1, "matern12"), (2, "rbf"), (3, "matern32"), (2, "matern52")):
        gp, rng = _synthetic(N, D, kind, 1000 * N + D)
        P, T = 5, 5
        y0 = np.ascontiguousarray(rng.uniform(0.1, 0.9, (P, D)))
        z = rng.standard_normal((P, T, D))
        nugget = gp._noise
        out = _samp(None, gp, y0, z, dt=0.05)
        what = f"N = {N}, D = {D}, {kind}"
        assert np.all(out["steps_done"] == T) and np.all(out["status"] == SR.CONVERGED), what
        cov_of = None
        if N > PR.LML_CHECK_MAX_N:
            def cov_of(x, gp=gp):
                C = np.asarray(gp.predict(np.ascontiguousarray(x), return_cov=True)[1], dtype=np.float64)
                C = C[..., 0] if C.ndim == 3 else C
                return C.astype(LD), 2 * PR.MARGIN * PR.FLOOR_ULPS + 4 * (T + 1)
        _check_factor(out, gp, kind, nugget, what, cov_of=cov_of)
        _check_pvar(out, gp, nugget, what)
        _check_velocity(out, z, 0.05, what)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [0, 1, 2, 63, 64, 65, 256])
def test_row_chunk_edges(T):
    """The steps at which a factor row gains a register chunk (64 lanes each), and the longest admitted path; N = 64, D = 2."""
    gp, rng = _synthetic(64, 2, "matern52", 77)
    P = 3
    y0 = np.ascontiguousarray(rng.uniform(0.1, 0.9, (P, 2)))
    z = rng.standard_normal((P, T, 2))
    out = _samp(None, gp, y0, z, dt=0.05)
    assert out["path"].shape == (P, T + 1, 2) and out["chol"].shape == (P, T, T) and out["cvar"].shape == (P, T)
    assert np.all(out["steps_done"] == T) and np.all(out["status"] == SR.CONVERGED)
    assert_array_equal(out["path"][:, 0], y0)
    _check_factor(out, gp, "matern52", gp._noise, f"T = {T}")
    if T:
        _check_pvar(out, gp, gp._noise, f"T = {T}")
        _check_velocity(out, z, 0.05, f"T = {T}")


@pytest.mark.gpu
def test_tile_column_edges():
    """P = 1, 15, 16, 17, 33: a tile partly filled, filled, one more, and a third workgroup; every path equals itself in the
    largest call, and the largest call is right."""
    gp, rng = _synthetic(64, 2, "rbf", 78)
    T = 5
    y0 = np.ascontiguousarray(rng.uniform(0.1, 0.9, (33, 2)))
    z = rng.standard_normal((33, T, 2))
    base = _samp(None, gp, y0, z, dt=0.05)
    _check_factor(base, gp, "rbf", gp._noise, "P = 33")
    _check_velocity(base, z, 0.05, "P = 33")
    for P in (1, 15, 16, 17):
        _same(_samp(None, gp, y0[:P], z[:P], dt=0.05), {k: v[:P] for k, v in base.items()}, f"P = {P}")


# ------------------------------------------------------------------------------------------------------------ 4. independence
@pytest.mark.gpu
def test_independence(letter2, monkeypatch):
    """A path's every output does not depend on P, on the others, on their order, on its column of the tile, on where the launches
    are cut or on the chunks of the host call."""
    chain, dyn = letter2["chain"], letter2["gp_dyn"]
    y0, X = _letter_starts(letter2["g"])
    z = _normals(M9, T12, 2, 9)
    run = lambda idx, **kw: _samp(chain, dyn, ys[idx], zs[idx], dt=0.5, x0=xs[idx], rtol=RTOL, **kw)
    # 9 paths of interest and 32 others (the same starts with other normals: other paths)
    others = np.arange(32) % M9
    ys, xs = np.concatenate([y0, y0[others]]), np.concatenate([X, X[others]])
    zs = np.concatenate([z, _normals(32, T12, 2, 10)])
    first = np.arange(M9)
    base = run(first)
    assert np.any(base["steps_done"] == T12)
    for m in range(M9):                                          # alone
        _same_path(run(np.array([m])), 0, base, m, f"path {m} alone")
    every = np.arange(M9 + 32)
    among = run(every)                                           # among 32 others: three workgroups
    for m in range(M9):
        _same_path(among, m, base, m, f"path {m} among 32 others")
    rev = run(every[::-1])                                       # reversed: other columns, other workgroups
    for m in range(M9 + 32):
        _same_path(rev, M9 + 32 - 1 - m, among, m, f"path {m} reversed")
    shifted = run(np.concatenate([every[5:22], first]))          # another tile column: 17 paths ahead
    for m in range(M9):
        _same_path(shifted, 17 + m, base, m, f"path {m} in another column")
    for per in ("1", "7"):                                       # the launch cuts (read per call)
        monkeypatch.setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", per)
        _same(run(every), among, f"{per} steps per launch")
    monkeypatch.delenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")
    monkeypatch.setenv("GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES", "1")  # the host chunks: one workgroup each, so 41 paths are 3 chunks
    _same(run(every), among, "three host chunks")
    monkeypatch.setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", "5")
    _same(run(every), among, "three host chunks, 5 steps per launch")
    monkeypatch.delenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")
    monkeypatch.delenv("GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES")
    # sample j of start m does not depend on S or M when the normals are sliced accordingly
    zz = np.random.RandomState(2).standard_normal((4, 6, T12, 2))
    full_path, full = chain.rollout_samples(dyn, y0[:4], T12, n_samples=6, dt=0.5, normals=zz, x0=X[:4], return_info=True, rtol=RTOL)
    assert full_path.shape == (4, 6, T12 + 1, 2) and full["cvar"].shape == (4, 6, T12) and full["status"].shape == (4, 6)
    part_path, part = chain.rollout_samples(dyn, y0[1:3], T12, n_samples=2, dt=0.5, normals=zz[1:3, 3:5], x0=X[1:3], return_info=True, rtol=RTOL)
    assert_array_equal(part_path, full_path[1:3, 3:5])
    for k in part:
        assert_array_equal(part[k], full[k][1:3, 3:5], err_msg=k)
    # the default draws are RandomState(random_state)'s
    seeded = chain.rollout_samples(dyn, y0[:4], T12, n_samples=6, dt=0.5, random_state=2, x0=X[:4], rtol=RTOL)
    assert_array_equal(seeded, full_path)


@pytest.mark.gpu
def test_beside_paths_that_end_early(letter2):
    """The letter-S fold starts with max_passes = 1 (test_rollout_stabilised._fold_starts: four end at step 0 with MAX_PASSES), and,
    without maps, one start at the edge of the doubles whose next point overflows: the survivors equal themselves run alone and
    the ended ones their own runs."""
    chain, dyn = letter2["chain1"], letter2["gp_dyn"]
    y0, x0, solver = _fold_starts(letter2)
    order = np.array([0, 4, 5, 6, 1, 2, 3, 7])
    z = _normals(len(order), T12, 2, 12)
    run = lambda idx: _samp(chain, dyn, y0[order[idx]], z[idx], dt=0.5, x0=x0[order[idx]], **solver)
    both = run(np.arange(len(order)))
    print(f"early ends: steps done {list(both['steps_done'])}, status {list(both['status'])}")
    assert np.all(both["steps_done"][[0, 4, 5, 6]] == 0) and np.all(both["status"][[0, 4, 5, 6]] == 1)      # INV_MAX_PASSES
    assert np.all(both["steps_done"][[1, 2, 3, 7]] >= 1)
    _check_nan_layout(both)
    for pos in range(len(order)):
        _same_path(run(np.array([pos])), 0, both, pos, f"place {pos}")
    # the overflow: dt = 1e306 and a start within 1e306 of the largest double, its first normals positive
    P, T = 6, 4
    ys = np.ascontiguousarray(letter2["g"]["demo"][::70][:P])
    ys[2] = [1.797e308, 1.0]
    zz = _normals(P, T, 2, 13)
    zz[2, 0] = [3.0, 0.0]
    out = _samp(None, dyn, ys, zz, dt=1e306)
    assert out["steps_done"][2] == 0 and out["status"][2] == SR.CONVERGED and np.all(np.isnan(out["path"][2, 1:]))
    assert np.all(np.isfinite(out["vel"][2, 0])) and np.all(out["steps_done"][[0, 1, 3, 4, 5]] == T)
    _check_nan_layout(out)
    for p in range(P):
        _same_path(_samp(None, dyn, ys[p:p + 1], zz[p:p + 1], dt=1e306), 0, out, p, f"overflow neighbour {p}")


# ------------------------------------------------------------------------------------------------------------ 5. degenerate
@pytest.mark.gpu
@pytest.mark.parametrize("kind", PR.KINDS)
def test_degenerate_end(kind, letter_kernels):
    gps, g = letter_kernels
    gp = gps[kind]
    P = 5
    y0 = np.ascontiguousarray(g["demo"][::80][:P])
    out = _samp(None, gp, y0, _normals(P, 6, 2, 1), nugget=0.0, dt=1e-300)
    assert_array_equal(out["x"][:, 1], out["x"][:, 0])
    assert np.all(out["steps_done"] == 1) and np.all(out["status"] == SR.DEGENERATE)
    floor = SR.floor(gp._c, 0.0)
    assert np.all(out["cvar"][:, 0] > floor) and np.all(~(out["cvar"][:, 1] > floor))
    _check_nan_layout(out)
    ok = _samp(None, gp, y0, _normals(P, 64, 2, 1), dt=1e-300)  # nugget = the noise level: the same points are no trouble
    assert np.all(ok["steps_done"] == 64) and np.all(ok["status"] == SR.CONVERGED)
    assert np.all(ok["cvar"] >= gp._noise - floor)


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def _raw(stages, hd, M, T, y0, x0, normals, outs, nugget=0.01, K=None, dt=0.5, rtol=RTOL, max_passes=64, entry="gpt_rollout_sampled",
         dev_arrays=False):
    """The C entry point itself on numpy arrays, as tests/test_rollout_stabilised.py::_raw.  Returns (rc, message).  The device
    entry gets NULL for every array unless dev_arrays: then it gets the addresses of the host arrays, for the refusals that look
    at which arrays are there (a refused call reads and writes none of them)."""
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
    y_, x0_, z_ = _lib.dptr(y0), _lib.dptr(x0), _lib.dptr(normals)
    if entry.endswith("_dev") and not dev_arrays:  # (every refusal asked of the device entry comes before it looks at an array)
        ptr, y_, x0_, z_ = (lambda k: None), None, None, None
    rc = getattr(_lib.load(), entry)(arr, (len(stages) if stages is not None else 0) if K is None else K, None if hd is None else hd._h, y_, x0_, z_,
                                     M, T, float(dt), float(rtol), int(max_passes), float(nugget), *(ptr(k) for k in _lib.ROLLOUT_SAMPLED_OUTPUTS))
    return rc, _lib.last_error()


def _sampled_sentinels(M, T, D):
    return dict(_sentinels(M, T, D), f=np.full((M, T, D), SENT), pvar=np.full((M, T), SENT), cvar=np.full((M, T), SENT),
                chol=np.full((M, T, T), SENT))


@pytest.mark.gpu
def test_refusals_and_models_untouched(letter2):
    from gaussian_process_transportation_amd import _lib
    case = letter2
    hd, stages = case["gp_dyn"]._handle, _stage_tuples(case)
    chain, gp_dyn = case["chain"], case["gp_dyn"]
    y = np.ascontiguousarray(case["g"]["traj"][:4])
    z = _normals(4, 3, 2, 0)
    probes = [m._handle for m in case["maps"]] + [hd]
    before = [h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd) for h in probes]
    _samp(chain, gp_dyn, y, z)
    outs = _sampled_sentinels(4, 3, 2)

    def refused(match, st=stages, hhd=hd, M=4, T=3, drop=(), code=_lib.GPT_E_ARG, dev=True, normals=z, **kw):
        for entry in ("gpt_rollout_sampled",) + (("gpt_rollout_sampled_dev",) if dev else ()):
            rc, msg = _raw(st, hhd, M, T, y, None, normals, {k: v for k, v in outs.items() if k not in drop}, entry=entry, **kw)
            assert rc == code and match in msg, (entry, match, rc, msg)
        assert all(_untouched(v) for v in outs.values()), match

    rng = np.random.default_rng(0)
    X2 = rng.uniform(0, 1, (30, 2))
    big = rng.uniform(0, 1, (1025, 2))
    large = _fit_gp(big, 0.05 * np.sin(big), 0.1, [0.3], 1e-2)
    refused("1025 training points", hhd=large._handle)
    refused("at most 1024", st=None, K=0, hhd=large._handle)
    refused("n_steps must be at most 256", T=257)
    refused("n_steps must be at most 256", st=None, K=0, T=257)
    for bad in (-1e-3, -1.0, float("nan"), float("inf"), -float("inf")):
        refused("nugget must be finite and >= 0", nugget=bad)
    for bad in (float("nan"), float("inf")):
        zb = z.copy()
        zb[3, 2, 1] = bad
        refused("normals contain NaN or infinity", normals=zb, dev=False)
    refused("normals must not be NULL", normals=None, dev=False)
    f32 = _fit_gp(X2, 0.05 * np.sin(X2), 0.1, [0.3], 1e-3, dtype="float32")
    refused("fp64 models only (the dynamics", hhd=f32._handle)
    multi = _lib.Handle(0)
    Z = rng.uniform(0, 1, (12, 2))
    A_ = rng.standard_normal((2, 12, 12))
    Sigma = np.ascontiguousarray(A_ @ A_.transpose(0, 2, 1) / 12 + 0.1 * np.eye(12))
    multi.fit_svgp(Z, rng.standard_normal((2, 12)), Sigma, np.array([0.3, 0.3]), np.array([1.0, 0.8]), 1e-2)
    refused("single-task models only (the dynamics", hhd=multi)
    # the mean rollout's own, in the same words
    refused("K must be 0 .. 4", K=5)
    refused("NULL handle (dynamics)", hhd=None)
    refused("n_steps must be >= 0", T=-1)
    refused("dt must be finite and not zero", dt=0.0)
    refused("rtol", rtol=0.0)
    refused("below 2^31", M=2 ** 23, T=255)                      # P (T + 1) = 2^31
    for name in ("path", "steps_done", "status"):
        refused("must not be NULL", drop=(name,), dev=False)
    # the device entry: valid models and every array NULL; every required array there but one; all there but the normals
    rc, msg = _raw(stages, hd, 4, 3, y, None, z, outs, entry="gpt_rollout_sampled_dev")
    assert rc == _lib.GPT_E_ARG and "y0, path, steps_done and status must not be NULL" in msg, (rc, msg)
    for name in ("path", "steps_done", "status"):
        rc, msg = _raw(stages, hd, 4, 3, y, None, z, {k: v for k, v in outs.items() if k != name}, entry="gpt_rollout_sampled_dev", dev_arrays=True)
        assert rc == _lib.GPT_E_ARG and "must not be NULL" in msg, (name, rc, msg)
    rc, msg = _raw(stages, hd, 4, 3, y, None, None, outs, entry="gpt_rollout_sampled_dev", dev_arrays=True)
    assert rc == _lib.GPT_E_ARG and "normals must not be NULL" in msg, (rc, msg)
    assert all(_untouched(v) for v in outs.values())
    # the Python front ends refuse the same before any device call
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="nugget must be finite and >= 0"):
            chain.rollout_samples(gp_dyn, y, 3, nugget=bad)
        with pytest.raises(ValueError, match="nugget must be finite and >= 0"):
            gp_dyn.rollout_samples(y, 3, nugget=bad)
    with pytest.raises(ValueError, match="1025 training points"):
        large.rollout_samples(y, 3)
    with pytest.raises(ValueError, match="1025 training points"):
        chain.rollout_samples(large, y, 3)
    with pytest.raises(ValueError, match="ROLLOUT_SAMPLED_MAX_T"):
        gp_dyn.rollout_samples(y, 257)
    with pytest.raises(ValueError, match="NaN or infinity"):
        gp_dyn.rollout_samples(y, 3, n_samples=1, normals=np.full((4, 1, 3, 2), np.nan))
    with pytest.raises(ValueError, match="normals has shape"):
        gp_dyn.rollout_samples(y, 3, n_samples=2, normals=np.zeros((4, 1, 3, 2)))
    with pytest.raises(NotImplementedError, match="float64 models only"):
        f32.rollout_samples(X2[:3], 2)
    # optional outputs: what was not asked for is not written, the rest does not change
    base = _samp(chain, gp_dyn, y, z, dt=0.5, rtol=RTOL)
    for asked in ((), ("chol",), ("vel", "cvar"), ("x", "f", "pvar"), ("vel", "x", "f", "pvar", "cvar", "chol")):
        o = _sampled_sentinels(6, 3, 2)
        rc, msg = _raw(stages, hd, 4, 3, y, None, z, {k: v for k, v in o.items() if k in asked or k in ("path", "steps_done", "status")},
                       nugget=gp_dyn._noise)
        assert rc == _lib.GPT_OK, msg
        for k in ALL_NAMES:
            if k in asked or k in ("path", "steps_done", "status"):
                assert_array_equal(o[k][:4], base[k], err_msg=f"{k} with {asked}")
                assert _untouched(o[k][4:]), k
            else:
                assert _untouched(o[k]), k
    rc, _ = _raw(stages, hd, 0, 3, y, None, z, outs)             # M = 0 does nothing
    assert rc == _lib.GPT_OK and all(_untouched(v) for v in outs.values())
    multi.close()
    for h, was in zip(probes, before):                           # every model predicts exactly what it did before
        now = h.predict_all(y, mean=True, var=True, J=True, Jvar=h is not hd)
        for k in was:
            if was[k] is not None:
                assert_array_equal(now[k], was[k], err_msg=k)
