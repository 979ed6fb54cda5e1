"""The residue (int8) variance product on the CPU: the numpy restatement (tests/var_int8_restatement.py) against Python big
integers and against an 80-bit product, and the host-side work split of the kernel (csrc/gpt_plan_i8.h) replayed by a
small program of its own.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import gp_oracle as orc
from tests import var_int8_bound as vb
from tests import var_int8_restatement as r8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc")


def test_moduli_are_coprime_and_fit_int8():
    for i, a in enumerate(r8.MODULI):
        assert a <= 256
        for b in r8.MODULI[i + 1:]:
            assert np.gcd(a, b) == 1
    assert abs(np.log2(float(r8.modulus_product())) - 110.16) < 0.01
    for m in r8.MODULI:
        res = r8.balanced(np.arange(-1000, 1000), m)
        assert res.min() >= -128 and res.max() <= 127
        assert np.all((res - np.arange(-1000, 1000)) % m == 0)


def test_bits_per_operand():
    assert r8.bits(512) == 50 and r8.bits(1024) == 49 and r8.bits(1536) == 49
    assert r8.bits(8192) == 48 and r8.bits(16384) == 47
    for NP in (512, 8192, r8.MAX_NP):
        assert NP * 4 ** r8.bits(NP) < r8.modulus_product() // 2        # no wrap-around
        assert r8.bits(NP) >= r8.MIN_BITS


def exact_product(A, B):
    return np.array([[sum(int(a) * int(b) for a, b in zip(row, col)) for col in B.T] for row in A], dtype=object)


@pytest.mark.parametrize("NP", [512, r8.MAX_NP])
def test_rebuilt_integer_is_exact_at_the_worst_case(NP):
    """every entry +-2^p, K = NP: the largest sums the scheme has to carry, both signs, and mixed signs that cancel"""
    p = r8.bits(NP)
    big = np.int64(1) << p
    A = np.stack([np.full(NP, big), np.full(NP, -big), np.where(np.arange(NP) % 2 == 0, big, -big), np.full(NP, big - 1)])
    B = np.stack([np.full(NP, big), np.full(NP, -big), np.where(np.arange(NP) % 3 == 0, big, -big)], axis=1)
    got = r8.integer_product(A, B, exact=True)
    want = exact_product(A, B)
    assert np.all(got == want)
    assert int(got[0, 0]) == NP * (1 << (2 * p)) and int(got[0, 1]) == -NP * (1 << (2 * p))
    np.testing.assert_allclose(r8.integer_product(A, B).astype(np.float64), want.astype(np.float64), rtol=2e-15, atol=0)


def test_rebuilt_integer_is_exact_on_random_operands():
    rng = np.random.default_rng(5)
    NP, p = 1536, r8.bits(1536)
    A = rng.integers(-(1 << p), (1 << p) + 1, (6, NP), dtype=np.int64)
    B = rng.integers(-(1 << p), (1 << p) + 1, (NP, 5), dtype=np.int64)
    A[1] >>= 30
    B[:, 2] >>= 40                     # small operands: the leading digits vanish
    B[:, 3] = 0
    got = r8.integer_product(A, B, exact=True)
    assert np.all(got == exact_product(A, B))
    ref = exact_product(A, B).astype(np.float64)
    np.testing.assert_allclose(r8.integer_product(A, B), ref, rtol=2e-15, atol=0)


@pytest.fixture(scope="module")
def model_1024():
    N, M = 1024, 64
    X, Y, Xq = orc.synthetic_problem(N, M)
    c, ls, noise, jit = 0.1, np.array([0.1, 0.1, 0.1]), 1e-4, 1e-10
    L, _ = orc.gpr_fit(X, Y, c, ls, noise, jit)
    W = solve_triangular(L, np.eye(N), lower=True, check_finite=False)
    Kst = orc.kernel_cross(Xq, X, c, ls).T.copy()
    V = (W.astype(np.longdouble) @ Kst.astype(np.longdouble))
    ref = (np.longdouble(c) + np.longdouble(noise) - np.sum(V * V, axis=0)).astype(np.float64)
    return dict(W=W, Kst=Kst, c=c, noise=noise, ref=ref, NP=1024)


def test_variance_against_an_80_bit_product(model_1024):
    """N = 1024, M = 64, synthetic_problem: |var - longdouble| <= 1e-12 — and the choice of the column exponent"""
    m = model_1024
    err = {}
    for how in ("prior", "column"):
        err[how] = float(np.max(np.abs(r8.variance(m["W"], m["Kst"], m["c"], m["noise"], m["NP"], how) - m["ref"])))
    fp64 = m["W"] @ m["Kst"]
    err["fp64"] = float(np.max(np.abs(m["c"] + m["noise"] - np.sum(fp64 * fp64, axis=0) - m["ref"])))
    print("max |var - longdouble|:", err)
    assert r8.COLUMN_EXPONENT == "prior"
    assert err["prior"] <= 1e-12
    assert err["column"] <= 1e-12


def test_fast_form_of_the_quantised_product_agrees(model_1024):
    m = model_1024
    a = r8.variance(m["W"], m["Kst"], m["c"], m["noise"], m["NP"])
    b = r8.variance_quantised(m["W"], m["Kst"], m["c"], m["noise"], m["NP"])
    assert np.max(np.abs(a - b)) <= 1e-13


def test_queries_far_from_the_data_quantise_to_zero():
    N = 512
    X, _, _ = orc.synthetic_problem(N, 4)
    c, ls, noise = 0.1, np.array([0.1, 0.1, 0.1]), 1e-4
    Kst = orc.kernel_cross(np.full((4, 3), 50.0), X, c, ls).T
    B, _ = r8.quantise_columns(Kst, r8.bits(N), c)
    assert np.all(B == 0)
    W = np.tril(np.random.default_rng(0).standard_normal((N, N)))
    assert np.all(r8.variance(W, Kst, c, noise, N) == c + noise)


# ---- the kernel's work split: every (column block, i-block) pair exactly once, whatever the batch size
PLAN_MAIN = r"""
#include "gpt_plan_i8.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    const long long ncols = atoll(argv[1]);
    const int nbi = atoi(argv[2]), P = atoi(argv[3]);
    const gpt::VarI8PlanDev d = gpt::build_var_i8_plan(ncols, nbi, P);
    printf("%lld %lld %d %d %d\n", (long long)d.ncb, (long long)d.nfull, d.nparts, gpt::var_i8_bits(nbi * 512), (int)gpt::var_i8_shape_ok(nbi * 512));
    for (int wg = 0; wg < P; ++wg) {
        int64_t cb; int lo, hi;
        if (gpt::var_i8_tail_item(d, wg, &cb, &lo, &hi)) printf("%d %lld %d %d\n", wg, (long long)cb, lo, hi);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("plan_i8")
    src = d / "plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = d / "plan_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("ncols,nbi,P", [(1, 3, 256), (128, 3, 256), (129, 3, 256), (33000, 3, 256), (500000, 16, 256),
                                         (10000, 16, 256), (16384, 16, 256), (200 * 128, 32, 256), (255 * 128, 1, 256), (700, 5, 7)])
def test_work_split_covers_every_pair_once(plan_program, ncols, nbi, P):
    out = subprocess.run([plan_program, str(ncols), str(nbi), str(P)], check=True, capture_output=True, text=True).stdout.split("\n")
    ncb, nfull, nparts, p, ok = (int(x) for x in out[0].split())
    assert ncb == -(-ncols // 128) and nfull == ncb // P * P and nfull % P == 0
    assert p == r8.bits(nbi * 512) and ok == 1
    seen = {}
    for line in out[1:]:
        if not line:
            continue
        wg, cb, lo, hi = (int(x) for x in line.split())
        assert nfull <= cb < ncb and 0 <= lo < hi <= nbi
        for ib in range(lo, hi):
            assert (cb, ib) not in seen
            seen[(cb, ib)] = wg
    assert len(seen) == (ncb - nfull) * nbi
    if ncb > nfull:
        assert nparts == min(P // (ncb - nfull), nbi)
        # balanced: no part of a block costs more than twice the mean (cost of an i-block: its tiles + 3)
        cost = {}
        for (cb, ib), wg in seen.items():
            cost[wg] = cost.get(wg, 0) + ib + 4
        mean = sum(cost.values()) / len(cost)
        assert max(cost.values()) <= 2 * mean + nbi + 4


# ---- the models of test_var_int8_gpu.py::test_other_shapes_kernels_and_scales: the quantisation bound, and the size of the bound the
# device is held to (tests/var_int8_bound.py has both derivations)
def cpu_model(pr):
    L, _ = orc.gpr_fit(pr["X"], pr["Y"], pr["c"], pr["ls"], pr["noise"], pr["jitter"], kind=pr["kind"])
    W = solve_triangular(L, np.eye(pr["N"]), lower=True, check_finite=False)
    Kst = orc.kernel_cross(pr["Xq"], pr["X"], pr["c"], pr["ls"], kind=pr["kind"]).T.copy()
    return W, Kst


@pytest.mark.parametrize("case", vb.CASES, ids=[c[0] for c in vb.CASES])
def test_restatement_meets_the_quantisation_bound_on_every_model(case):
    pr = vb.case_problem(case)
    W, Kst = cpu_model(pr)
    V = r8.product(W, Kst, pr["c"], pr["NP"])
    Wl, Kl = W.astype(np.longdouble), Kst.astype(np.longdouble)
    ref = Wl @ Kl
    # the reference's own error: N roundings of 2^-64 on sums of |W| |k|
    slack = (pr["N"] * 2.0 ** -63 * (np.abs(Wl) @ np.abs(Kl))).astype(np.float64) + vb.gamma(26) * np.abs(V)
    err = np.abs((V.astype(np.longdouble) - ref).astype(np.float64))
    bound = vb.quantisation_bound(W, Kst, pr["c"], pr["NP"]) + slack
    print(f"{pr['name']}: worst |dV| / bound {np.max(err / bound):.3f}, the bound is at most {bound.max():.2e} on |V| <= {np.abs(V).max():.2e}")
    assert np.all(err <= bound)
    dev = vb.device_bound(W, Kst, vb.kernel_rel_error(pr["X"], pr["Xq"], pr["ls"], pr["c"], pr["kind"]), pr["c"], pr["noise"], pr["NP"])
    print(f"{pr['name']}: device-against-restatement bound at most {dev.max():.2e} = {dev.max() / pr['c']:.2e} c")
    assert dev.max() <= 1e-10 * pr["c"]            # the bound says something: far below the 1e-5 of the oracle comparisons


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_derived_device_bound_is_below_the_fixed_tolerance_of_the_first_shape(kind):
    """N = 1300, c = 0.1, isotropic 0.1: test_var_int8_gpu.py holds this shape to 1e-12; the derived bound must be tighter"""
    pr = vb.case_problem(("first", 1300, 3, kind, (0.1, 0.1, 0.1), 0.1))
    pr["noise"], pr["jitter"] = 1e-4, 1e-10
    W, Kst = cpu_model(pr)
    dev = vb.device_bound(W, Kst, vb.kernel_rel_error(pr["X"], pr["Xq"], pr["ls"], pr["c"], kind), pr["c"], pr["noise"], pr["NP"])
    print(f"N = 1300 {kind}: derived bound at most {dev.max():.2e}")
    assert dev.max() < 1e-12
