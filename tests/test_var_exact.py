"""k_var (fp64 and fp32) and k_var_i8 on operands whose answer is known exactly (tests/var_exact_designs.py): one fit on the
design's lattice, then gpt_debug_set_inverse_factor puts the design's W in the place of the fit's L^-1, and both kernels run on
the same handle and queries (GPT_VAR_INT8 = 0 / 1).  Against the oracle at 1e-5 a dropped, doubled or misplaced (i, k) term of
a real model passes; here it changes a column by at least one unit of the design, and

  * k_var must return fl(fl(c + noise) - s2) BIT FOR BIT, fp64 and fp32: every partial sum of V and of sum V^2 is a multiple of
    one unit below 2^53 (2^24; Design.check_exact asserts it), so no order of summation, no cut of a sweep into partial
    products, no cohort and no ring depth can change a bit - only a wrong term can.
  * k_var_i8 must stay inside a DERIVED bound.  Its integer product C is exact, and the operands of these designs are exactly
    p-bit integers (Design.check_i8), so V_i = C 2^(e_i + f - 2p) but for the reconstruction: Horner in fp64 over 14 digits
    rounds up to 13 times (|C| >= 2^53 always, after scaling to p bits), |dV_i| <= gamma_13 |V_i|; the scalings by powers of two
    are exact.  The squares and their sum: i8_garner's value v enters ssq = fma(v, v, ssq), 16 per lane (4 row tiles x 4
    elements), then two shuffle additions (lanes +16, +32), then the 8 waves' partial sums are added in a row, then
    k_var_i8_finalize adds the nbi slots of the column: a fixed tree of depth d = 16 + 2 + 8 + nbi, so the computed sum is
    sum v^2 (1 + theta_d), |theta_d| <= gamma_d.  With v^2 = V^2 (1 + theta)^2, |(1 + theta)^2 - 1| <= 2 gamma_13 to first order:
        |s2' - s2| <= (2 gamma_13 + gamma_d) s2,
    and the last subtraction fl(fl(c + noise) - s2') adds u |c + noise - s2'| <= u (c + noise) (c + noise = 1 + 2^-6 is exact):
        |var - exact| <= (2 gamma_13 + gamma_d) s2 + u (c + noise),      u = 2^-53, gamma_k = k u / (1 - k u).
    That is 5e-15 s2 + 1.1e-16 at nbi = 1; one dropped F1 term is at least s2 / (64 N).  The worst error / bound of every case
    is printed.  (tests/test_var_exact_cpu.py holds the numpy restatement to the same bound.)

Plan features are asserted, not assumed: the fp64 plan through _lib.debug_var_plan for the device's workgroup count, the residue
plan by restating build_var_i8_plan's arithmetic; a feature none of the candidate batch sizes has FAILS the test.

This file: the k*-alone launch of single-task models with D <= 3, k_var and k_var_i8.  tests/test_var_exact_columns.py holds
the rest of k_var to the same kind of design: wide layouts (D = 4 .. 15, on a lattice whose every coordinate separates a pair
of sites) and multi-task models (gpt_debug_set_task_inverse_factor puts a design into each task's slot) bit for bit, and every
launch with derivative columns - whose operand is 0 on a site, so queries sit beside the sites and the generated operand is read
back from calibration runs (W = 2^e at one row per i-block) before the product is held to a derived bound of a few ulp.
Still not covered by exact designs: k_var_i8 beyond D <= 3 single-task (it takes nothing else), and more than one source per site
under derivative columns (the one-hot designs there make every V[i, m] a single product)."""
import functools
import os

import numpy as np
import pytest

from tests import var_exact_designs as vx
from tests import var_int8_restatement as r8

pytestmark = pytest.mark.gpu

KIND_NAMES = ("rbf", "matern12", "matern32", "matern52")
COUNTS = (1, 63, 64, 65, 127, 128, 129)


def padded(N):
    return -(-N // 512) * 512


@functools.lru_cache(maxsize=None)
def design(N, which, D=3, pow2=False):
    """pow2: the lattice of the Matern models (var_exact_designs.py: a distance of exactly 0 at every site)"""
    p = r8.bits(padded(N))
    kw = dict(D=D, pow2=pow2)
    return {"F1": lambda: vx.f1(N, **kw), "G1": lambda: vx.f2(N, 1, **kw), "G7": lambda: vx.f2(N, 7, **kw),
            "G7i": lambda: vx.f2(N, 7, interleaved=True, **kw), "G200": lambda: vx.f2(N, 200, **kw),
            "c8": lambda: vx.f2(N, -(-N // 8), offsets=(0, 1, 2), **kw), "c8i": lambda: vx.f2(N, -(-N // 8), interleaved=True, offsets=(0, 1, 2), **kw),
            "top1": lambda: vx.f2(N, 1, top_bits=p, **kw), "top5i": lambda: vx.f2(N, 5, interleaved=True, top_bits=p, **kw)}[which]()


@functools.lru_cache(maxsize=None)
def workgroups():
    """what gpt_api.hip's var_workgroups() takes as P: GPT_VAR_WGS, else the device's compute units"""
    e = os.environ.get("GPT_VAR_WGS")
    if e and int(e) > 0:
        return int(e)
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def model(d, kind=0, f32=False):
    """a handle fitted on the design's lattice (Y is arbitrary) whose inverse factor is the design's W"""
    from gaussian_process_transportation_amd import _lib
    h = _lib.Handle(0)
    if f32:
        h.set_dtype(_lib.GPT_F32)
    Y = np.cos(np.arange(d.N, dtype=np.float64))[:, None]
    h.fit(d.X, Y, np.ones(d.D), vx.C, vx.NOISE, 0.0, kernel_type=kind)
    h.debug_set_inverse_factor(d.W())
    return h


def run(h, d, qsite, monkeypatch, path):
    monkeypatch.setenv("GPT_VAR_INT8", str(path))
    v = h.predict_all(d.queries(qsite), var=True)["var"]
    assert h.var_path() == path
    return v


def check_kvar(h, d, qsite, monkeypatch, dtype=np.float64):
    got = run(h, d, qsite, monkeypatch, 0)
    want = d.expected(dtype)[qsite]
    assert got.dtype == dtype
    assert np.array_equal(got, want), vx.describe_wrong(d, qsite, got, want)


def check_i8(h, d, qsite, monkeypatch, worst):
    got = run(h, d, qsite, monkeypatch, 1)
    ratio, m = vx.i8_error_over_bound(d, padded(d.N) // 512, qsite, got)
    worst[0] = max(worst[0], ratio)
    if d.plain and not ratio <= 1.0:
        print(vx.describe_wrong(d, qsite, got, d.expected(np.float64)[qsite]))
    assert ratio <= 1.0, f"{d.name}: M = {len(qsite)}, |var - exact| is {ratio:.3g} of the bound at query {m} (site {qsite[m]})"


def both(h, d, qsite, monkeypatch, worst):
    if d.plain:
        check_kvar(h, d, qsite, monkeypatch)
    check_i8(h, d, qsite, monkeypatch, worst)


def small_batches(d):
    """1 .. 129 queries cycling over the sites with a stride (every count starts somewhere else), then one query per source"""
    out = [np.roll(vx.cycle_sites(d, d.n_sites + 1, 37), 11 * M)[:M] if M <= d.n_sites + 1 else vx.cycle_sites(d, M, 37) for M in COUNTS]
    out.append(d.site.copy())
    out.append(vx.cycle_sites(d, d.n_sites + 1))            # every site once, the empty ones and the origin
    return out


# ---- plan features --------------------------------------------------------------------------------------------------------------
def kvar_plan(M, nbi):
    from gaussian_process_transportation_amd import _lib
    return _lib.debug_var_plan(M, nbi, 1, workgroups())


def i8_plan(M, nbi):
    """build_var_i8_plan (csrc/gpt_plan_i8.h): column blocks of 128, whole rounds while P blocks are left, the tail's blocks get
    floor(P / ncb_t) workgroups each, at most nbi"""
    P = workgroups()
    ncb = -(-M // 128)
    nfull = ncb // P * P
    nparts = 0 if ncb == nfull else max(1, min(P // (ncb - nfull), nbi))
    return dict(ncb=ncb, nfull=nfull, nparts=nparts)


FEATURES = {
    "one_block": ((1, 40, 64), lambda k, i: k["ncb"] == 1 and i["ncb"] == 1),
    "tail_cut": ((460, 300, 700, 1000), lambda k, i: k["nfull"] == 0 and k["n_splits"] > 0 and k["cut_diag"] and i["nfull"] == 0 and i["nparts"] >= 1),
    "rounds_and_tail": ((33000, 50000, 40000, 70000), lambda k, i: 0 < k["nfull"] < k["ncb"] and 0 < i["nfull"] < i["ncb"]),
    "rounds_cut_diag": ((50000, 33000, 20000), lambda k, i: 0 < k["nfull"] < k["ncb"] and k["cut_diag"] and k["n_splits"] > 0 and 0 < i["nfull"] < i["ncb"]),
    "cohorts": ((9000, 14000, 12000, 10000, 16000, 8200), lambda k, i: k["cohorts"] and 128 <= k["ncb"] <= 255),
    "nbi16_whole_diag": ((8192, 10000, 16000), lambda k, i: not k["cut_diag"] and k["nfull"] == 0),
}


def pick(feature, nbi):
    cands, has = FEATURES[feature]
    for M in cands:
        if has(kvar_plan(M, nbi), i8_plan(M, nbi)):
            return M
    pytest.fail(f"no candidate batch size {cands} has the plan feature {feature} at nbi = {nbi} on {workgroups()} workgroups")


# ---- the hook itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [512, 1300])
def test_injected_factor_comes_back_bit_for_bit(N, monkeypatch):
    d = design(N, "F1")
    from gaussian_process_transportation_amd import _lib
    h = _lib.Handle(0)
    h.fit(d.X, np.ones((N, 1)), np.ones(3), vx.C, vx.NOISE, 0.0)
    h.lml()
    W = d.W()
    dirty = W + np.triu(np.full((N, N), 3.0), 1)             # the upper triangle is ignored, as the fit's packing ignores it
    h.debug_set_inverse_factor(dirty)
    back = h.export_inverse_factor()
    assert np.array_equal(np.tril(back), W)
    with pytest.raises(_lib.GptError):
        h.lml()                                              # L belongs to another matrix now
    check_kvar(h, d, d.site, monkeypatch)
    check_i8(h, d, d.site, monkeypatch, [0.0])
    h.fit(d.X, np.ones((N, 1)), np.ones(3), vx.C, vx.NOISE, 0.0)       # a new fit brings the model's own factor back
    h.lml()
    v = h.predict_all(d.queries(d.site[:64]), var=True)["var"]
    # K = (c + noise) I: 0.031, where the injected factor gives 1.0156 - s2 > 0.76 (which factor is in use, not a precision bound)
    assert np.max(np.abs(v - (vx.C + vx.NOISE - vx.C ** 2 / (vx.C + vx.NOISE)))) <= 1e-12
    h.close()


# ---- fp64 k_var and k_var_i8 ------------------------------------------------------------------------------------------------------
SMALL = [(N, w, k, 3) for N in (512, 1300) for k in range(4) for w in ("F1", "G1", "G7", "G7i", "top1", "top5i")]
SMALL += [(512, w, 0, D) for D in (1, 2) for w in ("F1", "G1", "G7i", "top5i")]
SMALL += [(N, w, 0, 3) for N in (1024, 2048) for w in ("F1", "G1", "G7i", "top1")]


@pytest.mark.parametrize("N,which,kind,D", SMALL, ids=lambda x: str(x))
def test_exact_designs_small_batches(N, which, kind, D, monkeypatch):
    d = design(N, which, D, pow2=kind != 0)
    d.check_i8(padded(N), r8.bits(padded(N)))
    h = model(d, kind)
    worst = [0.0]
    for qsite in small_batches(d):
        both(h, d, qsite, monkeypatch, worst)
    h.close()
    print(f"{d.name} {KIND_NAMES[kind]}: k_var_i8 worst error / bound {worst[0]:.3f}")


PLAN_CASES = [(512, "one_block"), (512, "rounds_and_tail"), (1024, "rounds_cut_diag"), (1024, "cohorts"), (1300, "one_block"),
              (1300, "tail_cut"), (1300, "rounds_and_tail"), (1300, "cohorts"), (2048, "tail_cut"), (2048, "cohorts"),
              (2048, "rounds_and_tail")]


@pytest.mark.parametrize("N,feature", PLAN_CASES)
def test_exact_designs_on_every_plan_feature(N, feature, monkeypatch):
    M = pick(feature, padded(N) // 512)
    worst = [0.0]
    for which in ("F1", "G7i"):
        d = design(N, which)
        h = model(d)
        both(h, d, vx.cycle_sites(d, M, 37 if which == "F1" else 1), monkeypatch, worst)
        h.close()
    print(f"N = {N}, {feature}: M = {M}, k_var_i8 worst error / bound {worst[0]:.3f}")


# ---- fp32 k_var ---------------------------------------------------------------------------------------------------------------------
F32 = [(N, "F1", k) for N in (512, 1300) for k in range(4)] + [(N, w, 0) for N in (512, 1300) for w in ("c8", "c8i")]


@pytest.mark.parametrize("N,which,kind", F32, ids=lambda x: str(x))
def test_exact_designs_fp32(N, which, kind, monkeypatch):
    d = design(N, which, pow2=kind != 0)
    nbi = padded(N) // 512
    h = model(d, kind, f32=True)
    assert h.model_info() == (1, 1)
    batches = small_batches(d)
    if kind == 0:
        rounds = next((M for M in (20000, 33000, 40000) if 0 < kvar_plan(M, nbi)["nfull"] < kvar_plan(M, nbi)["ncb"]), None)
        assert rounds is not None, "no candidate batch has whole rounds and a tail"
        batches += [vx.cycle_sites(d, 460, 37), vx.cycle_sites(d, rounds, 37)]
    for qsite in batches:
        check_kvar(h, d, qsite, monkeypatch, np.float32)
    h.close()


# ---- the production shape: N = 8192, 16 i-blocks, p = 48 -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_f1():
    d = design(8192, "F1")
    d.check_i8(8192, 48)
    h = model(d)
    yield d, h
    h.close()


@pytest.mark.parametrize("feature", ["nbi16_whole_diag", "cohorts", "rounds_and_tail", "tail_cut"])
def test_production_shape_one_hot(big_f1, feature, monkeypatch):
    d, h = big_f1
    M = pick(feature, 16)
    qsite = d.site.copy() if M == d.N else vx.cycle_sites(d, M, 37)
    worst = [0.0]
    both(h, d, qsite, monkeypatch, worst)
    print(f"{d.name}, {feature}: M = {M}, k_var_i8 worst error / bound {worst[0]:.3f}")


@pytest.mark.parametrize("which", ["G200", "G1", "top1"])
def test_production_shape_clusters(which, monkeypatch):
    d = design(8192, which)
    d.check_i8(8192, 48)
    h = model(d)
    worst = [0.0]
    for qsite in (vx.cycle_sites(d, d.n_sites + 1), vx.cycle_sites(d, 129, 3)):
        both(h, d, qsite, monkeypatch, worst)
    h.close()
    print(f"{d.name}: k_var_i8 worst error / bound {worst[0]:.3f}")
