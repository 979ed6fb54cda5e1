"""k_var_i8 after its work split changed: the images of the kernel columns come from a kernel of their own (k_i8_gen), and whole
groups of column blocks are dealt as (column block, i-block pair) items (csrc/gpt_plan_i8.h).  Every integer, every plane byte and
every fp64 sum stays what it was, and a (block, i-block) slot does not depend on who fills it: the outputs equal, bit for bit, what
the kernel computed before.

Fixture: tests/golden/var_i8_items_parent_bits.npz, written by tools/make_var_i8_items_parent_bits.py from a build of the commit
BEFORE the change (GPT_VAR_INT8=1): `var` at a seeded sample of 4096 queries that holds the first 256 and the last 256.  The outputs
do not depend on the work split, so the fixture does not depend on the CU count.  Shapes: the smallest that reach each new path on a
256-CU device, M = 33 000 = one whole group of 256 blocks plus a two-block tail:
  N = 2048              four i-blocks, two pairs
  N = 8192              sixteen i-blocks, eight pairs: the flagship's mapping, a workgroup keeps its pair
  N = 2500, Matern 3/2  NP = 2560, five i-blocks: odd, the middle one an item alone, padded rows
The N = 2048 result must not change with the launch split (item steps per launch 1 and more than a group has, one round per launch
exactly), and batches of M = 1 and M = 129 (columns past M repeat column M - 1 in the generating kernel) equal the leading entries of
the large batch."""
import os
import time

import numpy as np
import pytest

from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "var_i8_items_parent_bits.npz")
LS, C0, NOISE, JIT = np.array([0.1, 0.1, 0.1]), 0.1, 1e-4, 1e-10
M = 33000
NSAMPLE = 4096
CASES = (
    dict(id="N2048", kernel_type=0, N=2048),
    dict(id="N8192", kernel_type=0, N=8192),
    dict(id="N2500_matern32", kernel_type=2, N=2500),
)
SETTINGS = ("GPT_VAR_INT8", "GPT_VAR_ITEM_STEPS_PER_LAUNCH", "GPT_VAR_ROUNDS_EXACT", "GPT_VAR_ROUNDS_PER_LAUNCH")


def sample():
    """the queries whose `var` the fixture keeps: the first 256, the last 256, and a seeded draw of the rest, ascending"""
    rng = np.random.default_rng(20240611)
    mid = rng.choice(np.arange(256, M - 256), NSAMPLE - 512, replace=False)
    return np.sort(np.r_[0:256, mid, M - 256:M])


def problem(case):
    return orc.synthetic_problem(case["N"], M)


def fit(case):
    from gaussian_process_transportation_amd import _lib
    X, Y, _ = problem(case)
    h = _lib.Handle(0)
    h.fit(X, Y, LS, C0, NOISE, JIT, kernel_type=case["kernel_type"])
    return h


def var_i8(h, Xq, **settings):
    """var by the residue kernel under the given settings of the environment (read per call), which are put back afterwards"""
    old = {k: os.environ.get(k) for k in SETTINGS}
    try:
        for k in SETTINGS:
            os.environ.pop(k, None)
        os.environ["GPT_VAR_INT8"] = "1"
        os.environ.update(settings)
        var = h.predict_all(Xq, var=True)["var"]
        assert h.var_path() == 1, "the residue kernel did not take this launch"
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return var


def variance(case):
    """var of the case's M queries, and the seconds fit plus predict took"""
    t0 = time.perf_counter()
    h = fit(case)
    try:
        var = var_i8(h, problem(case)[2])
    finally:
        h.close()
    return var, time.perf_counter() - t0


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES[1:], ids=[c["id"] for c in CASES[1:]])
def test_bits_of_the_parent_build(case, golden):
    var, dt = variance(case)
    want = golden["var_" + case["id"]]
    got = var[sample()]
    print(f"{case['id']}: fit + predict {dt:.2f} s, var in [{var.min():.6g}, {var.max():.6g}], {int(np.sum(got != want))} of {got.size} differ")
    assert var.shape == (M,) and want.shape == (NSAMPLE,)
    assert np.all(np.isfinite(var)) and var.max() <= C0 + NOISE
    assert np.array_equal(got, want)


def test_bits_launch_splits_and_short_batches_at_2048(golden):
    case = CASES[0]
    Xq = problem(case)[2]
    h = fit(case)
    try:
        var = var_i8(h, Xq)
        want = golden["var_" + case["id"]]
        got = var[sample()]
        print(f"{case['id']}: var in [{var.min():.6g}, {var.max():.6g}], {int(np.sum(got != want))} of {got.size} differ")
        assert var.shape == (M,) and np.all(np.isfinite(var)) and var.max() <= C0 + NOISE
        assert np.array_equal(got, want)
        # two pairs: one item step per launch, and more than the group has
        assert np.array_equal(var, var_i8(h, Xq, GPT_VAR_ITEM_STEPS_PER_LAUNCH="1"))
        assert np.array_equal(var, var_i8(h, Xq, GPT_VAR_ITEM_STEPS_PER_LAUNCH="5"))
        assert np.array_equal(var, var_i8(h, Xq, GPT_VAR_ROUNDS_EXACT="1"))
        # the tail alone, its last block one column (M = 129) or the only block one column (M = 1): the other 127 are clamped
        for m in (1, 129):
            short = var_i8(h, Xq[:m])
            assert short.shape == (m,) and np.array_equal(short, var[:m])
    finally:
        h.close()
