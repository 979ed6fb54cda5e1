"""k_var_i8 after the order of its walk changed: a workgroup takes the i-blocks of an item two at a time and, inside such a group,
the moduli are the outer loop (csrc/gpt_plan_i8.h, "the walk of an item").  Every (column block, i-block) still writes its own slab
slot, and the integers, residues, Garner digits and fp64 sums per element are what they were: only the order in which a workgroup
visits (i-block, modulus) changed, so the outputs equal, bit for bit, what the kernel computed before.

Fixture: tests/golden/var_i8_modouter_parent_bits.npz, written by tools/make_var_i8_modouter_parent_bits.py from a build of the
commit BEFORE the change (GPT_VAR_INT8=1): `var` at a seeded sample of at most 4096 queries that holds the first 256 and the last 256.
The outputs do not depend on the work split, so the fixture does not depend on the CU count.  Shapes: the smallest at which each
form of the new walk occurs (256 workgroups):
  N =  512, M =    129   one i-block: a group of one; two tail blocks, the second of one column
  N = 1024, M = 33 000   two i-blocks: one pair per block, a whole group of 256 blocks plus a two-block tail
  N = 1536, M = 33 000   three i-blocks: the pair {2, 0} and the middle i-block alone; also with the Matern 3/2 kernel
  N = 4096, M = 12 800   eight i-blocks, the tail alone, 100 blocks in two parts
  N = 4096, M =  8 900   ... 70 blocks in three parts
At N = 4096 the two batch sizes together must give tail parts with an odd count >= 3 of i-blocks (twos and a single i-block left
over) and an even count >= 4 (several twos); the test asserts that from the plan, restated below from build_var_i8_plan and checked
against the header by tests/test_var_int8_modouter_cpu.py, so that another CU count fails instead of testing less.
Every case must give the same bits with all item steps of a group in one launch and with one, with one and two rounds per launch
where there are two rounds, and a batch and its two halves must agree."""
import os

import numpy as np
import pytest

from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "var_i8_modouter_parent_bits.npz")
LS, C0, NOISE, JIT = np.array([0.1, 0.1, 0.1]), 0.1, 1e-4, 1e-10
NSAMPLE = 4096
CASES = (
    dict(id="N512_M129", kernel_type=0, N=512, M=129),
    dict(id="N1024_M33000", kernel_type=0, N=1024, M=33000),
    dict(id="N1536_M33000", kernel_type=0, N=1536, M=33000),
    dict(id="N4096_M12800", kernel_type=0, N=4096, M=12800),
    dict(id="N4096_M8900", kernel_type=0, N=4096, M=8900),
    dict(id="N1536_M33000_matern32", kernel_type=2, N=1536, M=33000),
)
SETTINGS = ("GPT_VAR_INT8", "GPT_VAR_ITEM_STEPS_PER_LAUNCH", "GPT_VAR_ROUNDS_EXACT", "GPT_VAR_ROUNDS_PER_LAUNCH")


def sample(M):
    """the queries whose `var` the fixture keeps: the first 256, the last 256, and a seeded draw of the rest, ascending"""
    if M <= NSAMPLE:
        return np.arange(M)
    rng = np.random.default_rng(20241021)
    mid = rng.choice(np.arange(256, M - 256), NSAMPLE - 512, replace=False)
    return np.sort(np.r_[0:256, mid, M - 256:M])


def problem(case, M=None):
    return orc.synthetic_problem(case["N"], case["M"] if M is None else M)


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
    h = fit(case)
    try:
        return var_i8(h, problem(case)[2])
    finally:
        h.close()


# ---- the plan, restated (csrc/gpt_plan_i8.h build_var_i8_plan and the walk) ------------------------------------------------------
def workgroups():
    """what gpt_api.hip's var_workgroups() takes as P: GPT_VAR_WGS, else the device's compute units"""
    e = os.environ.get("GPT_VAR_WGS")
    if e and int(e) > 0:
        return int(e)
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def plan(M, nbi, P):
    """column blocks, those in whole rounds, and the i-block counts of a tail block's parts"""
    ncb = -(-M // 128)
    nfull = ncb // P * P
    if ncb == nfull:
        return dict(ncb=ncb, nfull=nfull, parts=[])
    nparts = max(1, min(P // (ncb - nfull), nbi))
    cost = [ib + 1 + 3 for ib in range(nbi)]                # var_i8_iblock_cost, I8_SWEEP_FIXED = 3
    total, bounds, ib, cum = sum(cost), [0], 0, 0
    for q in range(1, nparts):
        target = total * q // nparts
        lo, hi = bounds[q - 1] + 1, nbi - (nparts - q)
        while ib < hi and (ib < lo or cum + cost[ib] // 2 < target):
            cum += cost[ib]
            ib += 1
        bounds.append(ib)
    bounds.append(nbi)
    return dict(ncb=ncb, nfull=nfull, parts=[bounds[q + 1] - bounds[q] for q in range(nparts)])


def walk_groups(lo0, hi0, lo1, hi1):
    """the i-blocks of an item two at a time (var_i8_walk_iblock): a list of groups"""
    seq = list(range(hi0 - 1, lo0 - 1, -1)) + list(range(hi1 - 1, lo1 - 1, -1))
    return [seq[k:k + 2] for k in range(0, len(seq), 2)]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_cases_reach_every_form_of_the_walk():
    P = workgroups()
    pl = {c["id"]: plan(c["M"], c["N"] // 512, P) for c in CASES}
    print({k: v for k, v in pl.items()})
    a = pl["N512_M129"]
    assert a["nfull"] == 0 and a["ncb"] == 2 and a["parts"] == [1]                            # a group of one, tail only
    for k in ("N1024_M33000", "N1536_M33000", "N1536_M33000_matern32"):
        assert 0 < pl[k]["nfull"] < pl[k]["ncb"]                                            # a whole group plus a tail
    parts = pl["N4096_M12800"]["parts"] + pl["N4096_M8900"]["parts"]
    assert pl["N4096_M12800"]["nfull"] == 0 and pl["N4096_M8900"]["nfull"] == 0
    assert any(n % 2 == 1 and n >= 3 for n in parts), parts                                 # twos and one i-block left over
    assert any(n % 2 == 0 and n >= 4 for n in parts), parts                                 # several twos


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_bits_of_the_parent_build(case, golden):
    M, nbi = case["M"], case["N"] // 512
    Xq = problem(case)[2]
    h = fit(case)
    try:
        var = var_i8(h, Xq)
        want = golden["var_" + case["id"]]
        got = var[sample(M)]
        print(f"{case['id']}: var in [{var.min():.6g}, {var.max():.6g}], {int(np.sum(got != want))} of {got.size} differ")
        assert var.shape == (M,) and want.shape == got.shape
        assert np.all(np.isfinite(var)) and var.max() <= C0 + NOISE
        assert np.array_equal(got, want)
        # the launch split: one item step per launch (the default) and all of a group's; one round per launch exactly and two
        assert np.array_equal(var, var_i8(h, Xq, GPT_VAR_ITEM_STEPS_PER_LAUNCH="1"))
        assert np.array_equal(var, var_i8(h, Xq, GPT_VAR_ITEM_STEPS_PER_LAUNCH="0"))
        rounds = plan(M, nbi, workgroups())["nfull"] // workgroups()
        # (GPT_VAR_ROUNDS_EXACT = n: n rounds per launch whatever the shape; GPT_VAR_ROUNDS_PER_LAUNCH alone is scaled by the shape)
        assert np.array_equal(var, var_i8(h, Xq, GPT_VAR_ROUNDS_PER_LAUNCH="1", GPT_VAR_ROUNDS_EXACT="1"))
        if rounds >= 2:
            assert np.array_equal(var, var_i8(h, Xq, GPT_VAR_ROUNDS_PER_LAUNCH="2", GPT_VAR_ROUNDS_EXACT="2"))
        # a batch and its two halves
        half = M // 2
        assert np.array_equal(var[:half], var_i8(h, Xq[:half]))
        assert np.array_equal(var[half:], var_i8(h, Xq[half:]))
    finally:
        h.close()
