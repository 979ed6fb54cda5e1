"""Posterior and LML at the extremes of inputs and hyper-parameters, elementwise against tests/posterior_restatement.py.

The rest of the suite draws X from [0,1]^D, queries within 10 % of that box, c ~ 0.3 .. 20, l ~ 0.1 .. 10.  Here:
  a. queries on a ray leaving the data, until every k* has faded through the subnormals to exact zero (exp_tab's clamp, the
     fp32 exp2's underflow, ln c folded into the argument), for c = 1e-5, 1, 1e5;
  b. queries exactly on sources and 1e-9 l beside them (r = 0, sqrt(0), g(0); the variance cancels from c to about the noise);
  c. corners of the box the optimizer's restarts are drawn from: l = 30 x extent, l = spacing / 40, c / noise = 1e8, c = 1e-5
     with noise 1e-9, one long ARD length scale, with lml_gradient / lml_objective in both parametrisations;
  d. (X, Xq, l) against (2^k X, 2^k Xq, 2^k l), k = -20, +20: bitwise, since a power of two commutes with every rounding;
  e. X and Xq translated by 1000 x extent.
Layouts D = 1, 2 (rows of 4), 6 (rows of 8), 12 (rows of 16); O = 2; N = 300, and N = 600 (padded 1024) once per layout;
M >= 70 except on the sources (48).  Every model is asked for var alone, mean + J, Jvar alone and the fused J + Jvar + dvar.

fp64 bound: |library - longdouble| <= 16 max(e_ref, floor) per element (posterior_restatement: the rule, its scales and where
its numbers come from).  fp32 models: the exact and bitwise assertions of a and d, finiteness and var >= 0 everywhere; their
error is printed in units of the yardstick of test_kernel_dispatch.py.  Largest ratios seen on the MI355X: DESIGN.md section 2.

How the cases combine.  Sections a and c name a list per section (c values; theta corners) for every kernel type; the layouts
rotate through those lists so that every pair (layout, kernel type), (layout, c) and (layout, corner) occurs (but for D = 1 with the
ARD corner and with c / noise = 1e8, which is not admissible there: see CORNER), not every triple:
each reference costs about a second of 80-bit numpy and the whole module has a minute.  b, d and e take every (layout, kernel
type) pair.

Section a for the Matern kernels.  The exponential's argument is t = r, sqrt3 r, sqrt5 r, not h = r^2 / 2, and exp(-t) reaches
zero at t ~ 745, that is h ~ 9e4 .. 2.8e5.  The ray is therefore laid out in t (0 past 900, so h runs past 900 too, by far), and
`beyond h = 200` for the fp32 models reads `beyond t = 200` (the same thing for RBF): at h = 200 a Matern 5/2 k* is 1e-18 c,
which no arithmetic rounds to zero, while for t > 200 the fp32 argument (ln c - t) log2 e < -272 is below 2^-149 for every c."""
import functools

import numpy as np
import pytest

from tests import posterior_restatement as pr
from tests.posterior_restatement import KINDS, LD, G0

if not pr.longdouble_is_extended():
    pytest.skip(f"numpy.longdouble has eps {np.finfo(LD).eps:.2e} here (> 1e-18: no 80-bit extended type); the reference of these "
                "tests would be no better than the fp64 code it judges", allow_module_level=True)

JITTER = 1e-10
O = 2
LAYOUTS = (1, 2, 6, 12)
# var alone | k_mean_jac | Jacobian variance alone | fused with the cross products: out of REQUESTS of test_kernel_dispatch.py
REQUESTS = (dict(var=True), dict(mean=True, J=True), dict(Jvar=True), dict(J=True, Jvar=True, dvar=True))
REQUESTS_M12 = (dict(var=True), dict(mean=True))             # Matern 1/2 has no derivatives
C_VALUES = (1e-5, 1.0, 1e5)
CORNERS = ("long", "short", "big_c", "small_c", "ard_long")
# the ray of section a in the exponential's argument: coarse up to 690, 2.1 apart through every threshold (exact zero at
# 745 + ln c = 733.6 .. 756.6, subnormal from 708 + ln c on), coarse again past 900
RAY = np.concatenate([np.linspace(0.0, 690.0, 40, endpoint=False), np.linspace(690.0, 775.0, 40, endpoint=False),
                      np.linspace(775.0, 960.0, 20)])
F32_ZERO_ARG = 200.0


def requests(kt):
    return REQUESTS_M12 if kt == 1 else REQUESTS


def base_ls(D):
    """Length scales that keep cond(K) moderate: they grow with sqrt(D) as the distances do."""
    return 0.3 * max(1.0, np.sqrt(D / 3.0)) * np.linspace(0.8, 1.3, D)


def data(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, D))
    Y = np.stack([0.05 * np.sin(4.0 * X[:, o % D] + o) for o in range(O)], axis=1) + 0.01 * rng.standard_normal((N, O))
    return X, Y, rng


# --------------------------------------------------------------------------- the case list (fixed; nothing is skipped at run time)
FADE = [("fade", 300, LAYOUTS[(kt + ci) % 4], kt, c) for kt in range(4) for ci, c in enumerate(C_VALUES)] \
    + [("fade", 600, LAYOUTS[(kt + 3) % 4], kt, C_VALUES[kt % 3]) for kt in range(4)]
SOURCE = [("source", 300, D, kt, 1.3) for D in LAYOUTS for kt in range(4)]
# D of (kernel type, corner): the layouts rotate, but ARD needs D > 1, and c / noise = 1e8 on 300 points of a unit interval, or with
# the RBF kernel on the unit square, fails admission (cond(K) passes 1e10, or the fp64 restatement's gradient is off by more than
# 1e-9 of its scale)
#                 long  short  big_c  small_c  ard_long
CORNER_D = {0: (1,    2,     6,     12,      2),           # rbf
            1: (2,    6,     12,    1,       6),           # matern12
            2: (6,    12,    2,     2,       12),          # matern32
            3: (12,   1,     2,     6,       6)}           # matern52
CORNER = [("corner", 300, CORNER_D[kt][ti], kt, name) for kt in range(4) for ti, name in enumerate(CORNERS)]
SHIFT = [("shift", 300, D, kt, 1000.0) for D in LAYOUTS for kt in range(4)]
ALL_CASES = FADE + SOURCE + CORNER + SHIFT
SCALING = [(D, kt) for D in LAYOUTS for kt in range(4)]


def case_id(case):
    sec, N, D, kt, x = case
    return f"{sec}-N{N}-D{D}-{KINDS[kt]}-{x if isinstance(x, str) else format(x, 'g')}"


def ray_queries(X, ls, kind):
    """Queries x0 + s dhat in the scaled metric, x0 the source furthest out along dhat (it stays the nearest source: for every
    other source |q - X_n|^2 = s^2 + 2 s dhat.(x0 - X_n) + |x0 - X_n|^2 >= s^2), s chosen so that the exponential's argument at
    x0 takes the values of RAY."""
    D = X.shape[1]
    dhat = np.linspace(1.0, 0.5, D)
    dhat /= np.linalg.norm(dhat)
    Xs = X / ls
    x0 = Xs[np.argmax(Xs @ dhat)]
    s = {"rbf": np.sqrt(2.0 * RAY), "matern12": RAY, "matern32": RAY / np.sqrt(3.0), "matern52": RAY / np.sqrt(5.0)}[kind]
    return (x0[None, :] + s[:, None] * dhat[None, :]) * ls


def corner_theta(name, N, D):
    """(c, length scales as the fit takes them (1 or D), noise) of a corner; extent of the data: 1, spacing: N^(-1/D)."""
    c, noise, ls = 1.0, 1e-3, np.array([float(np.mean(base_ls(D)))])
    if name == "long":
        ls = np.array([30.0])
    elif name == "short":
        ls = np.array([N ** (-1.0 / D) / 40.0])
    elif name == "big_c":
        c, noise, ls = 1e5, 1e-3, (0.5 if D <= 2 else 1.0) * ls
    elif name == "small_c":
        c, noise = 1e-5, 1e-9
    elif name == "ard_long":
        ls = np.full(D, 0.2)
        ls[0] = 30.0
    else:
        raise ValueError(name)
    return c, ls, noise


@functools.lru_cache(maxsize=None)
def build(case):
    """Inputs and reference of a case, computed once per process, read-only."""
    sec, N, D, kt, x = case
    kind = KINDS[kt]
    X, Y, rng = data(N, D, 100 * D + kt + (7 if N == 600 else 0))
    c, ls, noise = 1.3, base_ls(D), 1e-3
    gradient = False
    if sec == "fade":
        c, noise = x, 1e-3 * x
        Xq = ray_queries(X, ls, kind)
    elif sec == "source":
        near = X[40:48].copy()
        for i in range(8):
            near[i, i % D] += 1e-9 * ls[i % D]
        Xq = np.concatenate([X[:40], near])
    elif sec == "corner":
        c, ls, noise = corner_theta(x, N, D)
        lsv = np.broadcast_to(ls, (D,))
        beside = X[:20] + 0.7 * lsv * np.where(np.arange(20)[:, None] % D == np.arange(D)[None, :], 1.0, 0.25)
        Xq = np.concatenate([beside, rng.uniform(-0.1, 1.1, (50, D))])
        gradient = True
    elif sec == "shift":
        X = X + x
        Xq = np.concatenate([X[:8], rng.uniform(-0.1, 1.1, (62, D)) + x])
    else:
        raise ValueError(sec)
    ref = pr.reference(X, Y, c, ls, noise, JITTER, kind, Xq, derivatives=kt != 1, gradient=gradient)
    g = dict(sec=sec, N=N, D=D, kt=kt, kind=kind, X=X, Y=Y, Xq=np.ascontiguousarray(Xq), c=c, ls=ls, noise=noise, ref=ref, id=case_id(case))
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def regions(g):
    """Section a: queries whose k* are all exactly zero as doubles, and queries with a subnormal k* (0 < k* < 2.2e-308)."""
    ks = g["ref"]["kstar"]
    return np.all(ks == 0.0, axis=1), np.any((ks > 0.0) & (ks < 2.2e-308), axis=1)


# --------------------------------------------------------------------------- CPU: the yardstick itself
def _close(a, b, what, rtol=1e-10):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.max(np.abs(b)))
    err = float(np.max(np.abs(a - b)))
    print(f"{what}: {err / scale:.2e} of the array scale")
    assert a.shape == b.shape and err <= rtol * scale, what


@pytest.mark.parametrize("kt", range(4), ids=KINDS)
def test_restatement_against_oracle_and_numpy_posterior(kt):
    from oracle import gp_oracle as orc
    from tests.test_matern_derivatives import np_posterior
    kind = KINDS[kt]
    X, Y, rng = data(120, 3, 5)
    Xq = rng.uniform(-0.1, 1.1, (30, 3))
    c, ls, noise = 0.7, np.array([0.35, 0.5, 0.4]), 1e-2
    ref = pr.reference(X, Y, c, ls, noise, JITTER, kind, Xq, derivatives=kt != 1)
    L, a = orc.gpr_fit(X, Y, c, ls, noise, JITTER, kind)
    mean, std = orc.gpr_predict(Xq, X, L, a, c, ls, noise, return_std=True, kind=kind)
    _close(ref["L"], L, "L")
    _close(ref["alpha"], a, "alpha")
    _close(ref["mean"], mean, "mean")
    _close(np.sqrt(ref["var"]), std[:, 0], "std")
    theta = np.log(np.concatenate([[c], ls, [noise]]))
    lml, grad = orc.log_marginal_likelihood(theta, X, Y, 3, JITTER, kind=kind)
    _close(ref["lml"], lml, "lml")
    _close(ref["grad_ard"], grad, "gradient (ARD)")
    iso = pr.reference(X, Y, c, ls[:1], noise, JITTER, kind)
    lml, grad = orc.log_marginal_likelihood(np.log([c, ls[0], noise]), X, Y, 1, JITTER, kind=kind)
    _close(iso["lml"], lml, "lml (isotropic)")
    _close(iso["grad_iso"], grad, "gradient (isotropic)")
    if kt == 0:
        o = orc.GaussianProcessOracle(c, ls, noise, JITTER).fit(X, Y)
        J, Jv = o.derivative(Xq, return_var=True)
        _close(ref["J"], J, "J")
        _close(ref["Jvar"], Jv[:, 0, :], "Jvar", 1e-9)          # the oracle inverts K explicitly
        _close(ref["dvar"], o.derivative_of_variance(Xq), "dvar", 1e-9)
    elif kt in (2, 3):
        m, v, J, Jvar, dvar = np_posterior(Xq, X, Y, c, ls, {2: 1.5, 3: 2.5}[kt], noise, JITTER)
        for key, b in (("mean", m), ("var", v), ("J", J), ("Jvar", Jvar), ("dvar", dvar)):
            _close(ref[key], b, key)
    for key in ref["e_rel"]:                                  # and the fp64 restatement of the library's algebra agrees too
        assert ref["e_rel"][key] <= 1e-11, key


def test_restatement_against_golden_fixtures():
    from tests.conftest import load_golden
    g = load_golden("synthetic_3d_N64")
    c, ls, noise = float(g["constant_value"]), g["length_scale"], float(g["noise_level"])
    ref = pr.reference(g["X"], g["Y"], c, ls, noise, float(g["alpha"]), "rbf", g["Xq"], gradient=False)
    _close(ref["L"], g["L_"], "L")
    _close(ref["alpha"], g["alpha_"], "alpha")
    _close(ref["mean"], g["mean"], "mean")
    _close(np.sqrt(ref["var"]) - np.sqrt(noise), g["std"][:, 0], "std")     # the reference class subtracts sqrt(noise)
    for th, v, gr in zip(g["lml_theta"], g["lml_value"], g["lml_grad"]):
        r = pr.reference(g["X"], g["Y"], np.exp(th[0]), np.exp(th[1:4]), np.exp(th[4]), float(g["alpha"]), "rbf")
        _close(r["lml"], v, "lml")
        _close(r["grad_ard"], gr, "gradient")
    g = load_golden("matern_5d")
    for tag, kind in (("12", "matern12"), ("32", "matern32"), ("52", "matern52")):
        for kk, ls, key in (("ard", g["length_scale"], "grad_ard"), ("iso", np.array([float(g["iso_length_scale"])]), "grad_iso")):
            pre = f"m{tag}_{kk}_"
            ref = pr.reference(g["X"], g["Y"], 0.3, ls, 0.01, 1e-10, kind, g["Xq"], derivatives=False, gradient=False)
            _close(ref["alpha"], g[pre + "alpha_"], pre + "alpha")
            _close(np.diag(ref["L"]), g[pre + "Ldiag"], pre + "diag L")
            _close(ref["mean"], g[pre + "mean"], pre + "mean")
            _close(np.sqrt(ref["var"]) - np.sqrt(0.01), g[pre + "std"][:, 0], pre + "std")
            th, v, gr = g[pre + "lml_theta"][0], g[pre + "lml_value"][0], g[pre + "lml_grad"][0]
            r = pr.reference(g["X"], g["Y"], np.exp(th[0]), np.exp(th[1:-1]), np.exp(th[-1]), 1e-10, kind)
            _close(r["lml"], v, pre + "lml")
            _close(r[key], gr, pre + "gradient")


ADMITTED = list(ALL_CASES)


def test_no_case_is_left_out():
    left_out = [c for c in ALL_CASES if c not in ADMITTED]
    assert len(left_out) <= 0
    assert len(FADE) == 16 and len(SOURCE) == 16 and len(CORNER) == 20 and len(SHIFT) == 16
    for D in LAYOUTS:                                        # the pairs the module's docstring promises
        assert {kt for s, N, d, kt, x in FADE if d == D} == set(range(4)) and {x for s, N, d, kt, x in FADE if d == D} == set(C_VALUES)
        assert sum(1 for s, N, d, kt, x in FADE if d == D and N == 600) == 1
        assert {x for s, N, d, kt, x in CORNER if d == D} >= set(CORNERS[:2] + CORNERS[3:4] + (CORNERS[2:3] if D > 1 else ()))
    assert {(kt, x) for s, N, d, kt, x in FADE} == {(kt, c) for kt in range(4) for c in C_VALUES}
    assert {(kt, x) for s, N, d, kt, x in CORNER} == {(kt, n) for kt in range(4) for n in CORNERS}


@pytest.mark.parametrize("case", ADMITTED, ids=case_id)
def test_admission(case):
    """The case is one the bound can be asked of: K factors in longdouble, cond(K) <= 1e10, every reference output is finite,
    e_ref <= 1e-9 of the scale, and the section's own premise holds."""
    g = build(case)
    ref = g["ref"]
    ev = np.linalg.eigvalsh(ref["K"])
    cond = float(ev[-1] / ev[0])
    print(f"{g['id']}: cond(K) {cond:.3e}; e_ref / scale " + ", ".join(f"{k} {v:.1e}" for k, v in ref["e_rel"].items()))
    assert ev[0] > 0 and cond <= 1e10
    for key in ("L", "alpha", "lml", "kstar") + tuple(k for k in pr.OUTPUTS + ("grad_ard", "grad_iso") if k in ref):
        assert np.all(np.isfinite(ref[key])), key
    for key, e in ref["e_rel"].items():
        assert e <= 1e-9, key
    assert len(g["Xq"]) >= (48 if g["sec"] == "source" else 70)
    if g["sec"] == "fade":
        zero, fading = regions(g)
        h_min = 0.5 * np.min(np.sum(((g["Xq"][:, None, :] - g["X"][None, :, :]) / g["ls"]) ** 2, axis=-1), axis=1)
        print(f"    {int(zero.sum())} queries with every k* exactly zero, {int(fading.sum())} with subnormal k*, h up to {h_min.max():.0f}")
        assert zero.sum() >= 5 and fading.sum() >= 3 and h_min.min() < 1e-20 and h_min.max() > 900.0
        assert np.all(ref["arg_min"][zero] > F32_ZERO_ARG) and (ref["arg_min"] > F32_ZERO_ARG).sum() > zero.sum()
    if g["sec"] == "source":
        assert g["noise"] >= 1e-6 * g["c"]
        assert np.all(ref["var"] > ref["tol"]["var"]) and np.all(ref["var"] < 3 * g["noise"])     # cancelled, and still resolved


# --------------------------------------------------------------------------- GPU
def fitted(g, dtype=0, X=None, ls=None):
    from gaussian_process_transportation_amd import _lib
    h = _lib.Handle(0)
    h.set_dtype(dtype)
    h.set_matern_derivatives(True)
    h.fit(g["X"] if X is None else X, g["Y"], g["ls"] if ls is None else ls, g["c"], g["noise"], JITTER, kernel_type=g["kt"])
    return h


def predict(h, Xq, kt):
    """[(flags, {name: array})] for every request of the kernel type."""
    outs = []
    for flags in requests(kt):
        out = h.predict_all(Xq, **flags)
        outs.append((flags, {k: v for k, v in out.items() if v is not None}))
    return outs


def hold_fp64(outs, g, worst):
    for flags, out in outs:
        for k, a in out.items():
            assert a.dtype == np.float64
            worst[k] = max(worst.get(k, 0.0), pr.assert_within(a, g["ref"], k, f"{g['id']} {sorted(flags)}"))


def finite_fp32(outs, g):
    """fp32 models outside the tame corner: every output finite (and var >= 0).  Their error is printed in units of the
    project's fp32 yardstick (2e-4 of the array scale, of the prior derivative variance for Jvar), not asserted: that yardstick
    was set for well-conditioned models, and on 300 points of a unit interval sum |k* alpha| is 1e3 times the mean."""
    ref = g["ref"]
    for flags, out in outs:
        for k, a in out.items():
            assert a.dtype == np.float32 and np.all(np.isfinite(a)), (k, flags)
            scale = float(np.max(ref["scale_Jvar"])) if k == "Jvar" else float(np.max(np.abs(ref[k])))
            err = float(np.max(np.abs(a.astype(np.float64) - ref[k])))
            print(f"{g['id']} fp32 {sorted(flags)} {k}: {err / scale:.2e} of the array scale (yardstick 2e-4)")
        if "var" in out:
            assert np.all(out["var"] >= 0), flags


def report(g, worst):
    print("RATIOS " + g["id"] + " " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


def prior_jvar(g, ty):
    """c (g(0) (1/l_d) (1/l_d)) as k_var_finalize forms it, in the model's element type."""
    inv = 1.0 / np.broadcast_to(g["ls"], (g["D"],))
    return ty(g["c"]) * (G0[g["kind"]] * inv * inv).astype(ty)


def hold_exact(outs, g, where, ty):
    """Where every k* is zero the posterior is the prior, to the bit."""
    assert where.sum() >= 5
    exact_prior(outs, g, where, ty)


def exact_prior(outs, g, where, ty):
    for flags, out in outs:
        if "mean" in out:
            assert np.all(out["mean"][where] == 0), flags
        if "var" in out:
            assert np.all(out["var"][where] == ty(g["c"]) + ty(g["noise"])), flags
        if "J" in out:
            assert np.all(out["J"][where] == 0), flags
        if "dvar" in out:
            assert np.all(out["dvar"][:, where] == 0), flags
        if "Jvar" in out:
            p = prior_jvar(g, ty)
            assert np.all(np.abs(out["Jvar"][where] - p) <= 2 * np.spacing(p)), flags


@pytest.mark.gpu
@pytest.mark.parametrize("case", FADE, ids=case_id)
def test_fading_and_vanished_kernel_values(case):
    from gaussian_process_transportation_amd import _lib
    g = build(case)
    zero, _ = regions(g)
    worst = {}
    h = fitted(g)
    try:
        outs = predict(h, g["Xq"], g["kt"])
    finally:
        h.close()
    hold_fp64(outs, g, worst)
    hold_exact(outs, g, zero, np.float64)
    report(g, worst)
    h = fitted(g, _lib.GPT_F32)
    try:
        outs = predict(h, g["Xq"], g["kt"])
    finally:
        h.close()
    finite_fp32(outs, g)
    hold_exact(outs, g, g["ref"]["arg_min"] > F32_ZERO_ARG, np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SOURCE, ids=case_id)
def test_queries_on_the_sources(case):
    from gaussian_process_transportation_amd import _lib
    g = build(case)
    worst = {}
    h = fitted(g)
    try:
        outs = predict(h, g["Xq"], g["kt"])
    finally:
        h.close()
    hold_fp64(outs, g, worst)
    var = outs[0][1]["var"]
    assert np.all(var >= 0) and np.all(var > 0.5 * g["ref"]["var"])       # the clamp at 0 did not stand in for the sum
    report(g, worst)
    h = fitted(g, _lib.GPT_F32)
    try:
        finite_fp32(predict(h, g["Xq"], g["kt"]), g)
    finally:
        h.close()


def lml_both_ways(h, g, ls, key, worst):
    """fit + lml_gradient, then lml_objective: the same bits, and value and every component within the rule."""
    h.fit(g["X"], g["Y"], ls, g["c"], g["noise"], JITTER, kernel_type=g["kt"])
    v0, g0 = h.lml_gradient(ls.size)
    v1, g1 = h.lml_objective(g["X"], g["Y"], ls, g["c"], g["noise"], JITTER, kernel_type=g["kt"])
    assert v0 == v1 and np.array_equal(g0, g1)
    what = f"{g['id']} n_ls={ls.size}"
    worst["lml"] = max(worst.get("lml", 0.0), pr.assert_within(np.float64(v0), g["ref"], "lml", what))
    worst["grad"] = max(worst.get("grad", 0.0), pr.assert_within(g0, g["ref"], key, what))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CORNER, ids=case_id)
def test_corners_of_the_optimizers_box(case):
    g = build(case)
    D, worst = g["D"], {}
    h = fitted(g)
    try:
        hold_fp64(predict(h, g["Xq"], g["kt"]), g, worst)
        if g["ls"].size == 1:
            lml_both_ways(h, g, g["ls"], "grad_iso", worst)
        if D > 1:                                            # the same model with a gradient component per coordinate
            lml_both_ways(h, g, np.ascontiguousarray(np.broadcast_to(g["ls"], (D,))), "grad_ard", worst)
    finally:
        h.close()
    report(g, worst)


def everything(dtype, kt, X, Y, Xq, ls, c, noise):
    from gaussian_process_transportation_amd import _lib
    h = _lib.Handle(0)
    try:
        h.set_dtype(dtype)
        h.set_matern_derivatives(True)
        h.fit(X, Y, ls, c, noise, JITTER, kernel_type=kt)
        got = dict(zip(("L", "alpha"), h.export()))
        got["lml"] = np.array(h.lml())
        for i, flags in enumerate(requests(kt)):
            got.update({f"{k}@{i}": v for k, v in h.predict_all(Xq, **flags).items() if v is not None})
        got["lml_of_gradient"], got["gradient"] = h.lml_gradient(ls.size)
        got["lml_of_gradient"] = np.array(got["lml_of_gradient"])
    finally:
        h.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("D,kt", SCALING, ids=[f"D{D}-{KINDS[kt]}" for D, kt in SCALING])
def test_power_of_two_rescaling_changes_no_bit(D, kt, dtype):
    """1 / l is correctly rounded, X (1 / l) has identical bits, sqrt2 / l scales exactly: L, alpha, LML, gradient, mean and
    var are unchanged and J, Jvar, dvar scale by 2^-k, 4^-k, 2^-k exactly."""
    X, Y, rng = data(300, D, 900 + 10 * D + kt)
    Xq = np.concatenate([X[:8], rng.uniform(-0.1, 1.1, (62, D))])
    ls, c, noise = base_ls(D), 1.3, 1e-2
    ref = everything(dtype, kt, X, Y, Xq, ls, c, noise)
    for v in ref.values():
        assert np.all(np.isfinite(v))
    for k in (-20, 20):
        s = 2.0 ** k
        got = everything(dtype, kt, s * X, Y, s * Xq, s * ls, c, noise)
        assert got.keys() == ref.keys()
        bad = []
        for key, a in got.items():
            name = key.split("@")[0]
            a = a * a.dtype.type({"J": s, "Jvar": s * s, "dvar": s}.get(name, 1.0))
            if not np.array_equal(a, ref[key]):
                d = np.abs(a.astype(np.float64) - ref[key].astype(np.float64))
                bad.append(f"{key}: {int((a != ref[key]).sum())} of {a.size} differ (max {d.max():.3e})")
        assert not bad, f"k = {k}: " + "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHIFT, ids=case_id)
def test_translated_inputs(case):
    """e_ref contains what scaling before subtracting costs at |x| = 1000 x extent; fp32 inputs have lost the digits already.

    The first 8 queries are sources, bit for bit, and the library does not put them at r = 0.  The stored sources are
    (x (1 / l)) (1 / sqrt2), a query is x ((1 / l)(1 / sqrt2)) with the product of the constants rounded once (k_mean_jac, k_var;
    the inverse-map, pull-back and chain units scale the same way): two roundings of one number, an ulp of |x / l| apart per
    coordinate, r ~ 1e-12 at |x / l| = 1600 and D = 12.  A power of two commutes with both (section d is bitwise) and a kernel
    that is smooth at r = 0 turns it into r^2; Matern 1/2, k = c (1 - r + ..), shows it in first order: var at a source is off
    by 2 c r ~ 2e-12.  Both roundings are within the error that any scaling before subtracting has away from the sources;
    posterior_float64 scales the way the library does, so e_ref carries that cost."""
    from gaussian_process_transportation_amd import _lib
    g = build(case)
    worst = {}
    h = fitted(g)
    try:
        outs = predict(h, g["Xq"], g["kt"])
    finally:
        h.close()
    hold_fp64(outs, g, worst)
    report(g, worst)
    h = fitted(g, _lib.GPT_F32)
    try:
        finite_fp32(predict(h, g["Xq"], g["kt"]), g)
    finally:
        h.close()


FAR = {0: 1e160, 1: 1e25}          # scaled distance whose square overflows the model's element type: h = +inf


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("D", [2, 6])
@pytest.mark.parametrize("kt", range(4), ids=KINDS)
def test_query_beyond_the_range_of_h(kt, D, dtype):
    """The last query is so far out that h itself overflows: ln c - h = -inf.  exp_tab's clamp at -800 (and exp2 of -inf in fp32)
    is what turns that into k* = 0 and the prior; without the clamp r = fma(n, -step, t) is inf - inf.  Matern 3/2 and 5/2
    multiply the exponential by a polynomial in t = sqrt(nu') r, which is inf there, and inf x 0 is NaN: gpt_exp.h bounds t
    (matern_bound) before both."""
    ty = (np.float64, np.float32)[dtype]
    X, Y, rng = data(40, D, 50 + D)
    ls = base_ls(D)
    Xq = rng.uniform(-0.1, 1.1, (70, D))
    Xq[-1] = FAR[dtype] * ls
    g = dict(X=X, Y=Y, ls=ls, c=0.5, noise=1e-2, kt=kt, kind=KINDS[kt], D=D)
    h = fitted(g, dtype)
    try:
        outs = predict(h, Xq, kt)
    finally:
        h.close()
    for flags, out in outs:
        for k, a in out.items():
            assert np.all(np.isfinite(a)), (k, flags)
    far = np.zeros(70, dtype=bool)
    far[-1] = True
    exact_prior(outs, g, far, ty)
