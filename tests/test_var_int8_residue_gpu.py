"""k_var_i8 after its residues moved from fp64 (quotient, fma, two compare / select fix-ups, conversions) to byte dot products with
one fp32 quotient (csrc/gpt_residue_i8.h): a residue is an exact integer either way, so every plane, every parked byte and every
output equals, bit for bit, what the kernel computed before.

Fixture: tests/golden/var_i8_residue_parent_bits.npz, written by tools/make_var_i8_residue_parent_bits.py from a build of the
commit BEFORE the change (GPT_VAR_INT8=1): `var` in full per case.  tests/test_var_int8_feed.py already holds RBF at N = 400, 1000
and 1300 to such a fixture; the cases here are what it does not reach:
  matern12 / 32 / 52   N = 1000 (NP = 1024: one full tile and the diagonal), M = 300 (a divided tail): the three generating
                       instantiations that had no bit fixture
  rbf_c_pow2           c = 0.125 = 2^f exactly, N = 400 (p = 50), M = 129, the first 16 queries copies of sources: where the
                       generated k* rounds to B' = 2^p, the operand's top byte (bit 50 of the integer) is in use
  rbf_N16384           the largest model the path takes: p = 47, 32 i-blocks, the largest accumulators"""
import os
import time

import numpy as np
import pytest

from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "var_i8_residue_parent_bits.npz")
LS, NOISE, JIT = np.array([0.1, 0.1, 0.1]), 1e-4, 1e-10
CASES = (
    dict(id="matern12", kernel_type=1, N=1000, M=300, c=0.1, copies=0),
    dict(id="matern32", kernel_type=2, N=1000, M=300, c=0.1, copies=0),
    dict(id="matern52", kernel_type=3, N=1000, M=300, c=0.1, copies=0),
    dict(id="rbf_c_pow2", kernel_type=0, N=400, M=129, c=0.125, copies=16),
    dict(id="rbf_N16384", kernel_type=0, N=16384, M=129, c=0.1, copies=0),
)


def problem(case):
    X, Y, Xq = orc.synthetic_problem(case["N"], case["M"])
    Xq[:case["copies"]] = X[:case["copies"]]
    return X, Y, Xq


def variance(case):
    """var of the case's queries by the residue kernel, and the seconds fit plus predict took"""
    from gaussian_process_transportation_amd import _lib
    X, Y, Xq = problem(case)
    h = _lib.Handle(0)
    old = os.environ.get("GPT_VAR_INT8")
    try:
        t0 = time.perf_counter()
        h.fit(X, Y, LS, case["c"], NOISE, JIT, kernel_type=case["kernel_type"])
        os.environ["GPT_VAR_INT8"] = "1"
        var = h.predict_all(Xq, var=True)["var"]
        dt = time.perf_counter() - t0
        assert h.var_path() == 1, "the residue kernel did not take this launch"
    finally:
        if old is None:
            os.environ.pop("GPT_VAR_INT8", None)
        else:
            os.environ["GPT_VAR_INT8"] = old
        h.close()
    return var, dt


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_bits_of_the_parent_build(case, golden):
    var, dt = variance(case)
    want = golden["var_" + case["id"]]
    print(f"{case['id']}: fit + predict {dt:.2f} s, var in [{var.min():.6g}, {var.max():.6g}], "
          f"{int(np.sum(var != want))} of {var.size} differ")
    assert var.shape == (case["M"],) and want.shape == (case["M"],)
    assert np.all(np.isfinite(var)) and var.max() <= case["c"] + NOISE
    assert np.array_equal(var, want)
