"""The walk of k_var_i8 through an item (csrc/gpt_plan_i8.h, var_i8_item_walk): the item's i-blocks two at a time, and inside such
a group the moduli outermost.  A small program of its own replays the items of a plan (var_i8_group_item, var_i8_tail_as_item) and
their walks on the CPU, under the address and undefined-behaviour sanitizers, as tests/test_var_int8_items_cpu.py replays the
items.  What the argument for the order rests on is asserted here: every pair item of a group of column blocks runs the same
number of tiles per modulus, so the workgroups that share a block's image stay in one plane of it.  No GPU."""
import os
import shutil
import subprocess

import pytest

from tests import test_var_int8_modouter_gpu as gpu_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc")

# first line: blocks, blocks in whole groups, pairs per block, park bytes per workgroup and per slot; then the bounds of the tail's
# parts; then one line per walk entry: kind (0 pair item, 1 tail part), item number, block, lo0 hi0 lo1 hi1, group, slot, i-block,
# tiles of the entry's group per modulus
WALK_MAIN = r"""
#include "gpt_plan_i8.h"
#include <cstdio>
#include <cstdlib>
static void walk(int kind, long long item, const gpt::VarI8Item& x) {
    const std::vector<gpt::VarI8WalkEntry> w = gpt::var_i8_item_walk(x);
    for (const gpt::VarI8WalkEntry& e : w)
        printf("%d %lld %lld %d %d %d %d %d %d %d %d\n", kind, item, (long long)x.cb, x.lo[0], x.hi[0], x.lo[1], x.hi[1], e.group, e.slot, e.ib,
               gpt::var_i8_group_tiles(w, e.group));
}
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const long long ncols = atoll(argv[1]);
    const int nbi = atoi(argv[2]), P = atoi(argv[3]);
    gpt::VarI8PlanDev d = gpt::build_var_i8_plan(ncols, nbi, P);
    const int npairs = gpt::var_i8_npairs(nbi);
    printf("%lld %lld %d %zu %zu\n", (long long)d.ncb, (long long)d.nfull, npairs, gpt::var_i8_park_bytes(), gpt::var_i8_park_slot_bytes());
    for (int q = 0; q <= d.nparts; ++q) printf("%d ", d.bounds[q]);
    printf("\n");
    long long item = 0;
    for (long long r = 0; r < d.nfull / P; ++r) {
        d.rnd_begin = r; d.rnd_end = r + 1;
        for (int k = 0; k < npairs; ++k)
            for (int wg = 0; wg < P; ++wg) walk(0, item++, gpt::var_i8_group_item(d, r, k, wg));
    }
    d.rnd_begin = d.rnd_end = d.nfull / P;
    for (int wg = 0; wg < P; ++wg) {
        gpt::VarI8Item x;
        if (gpt::var_i8_tail_as_item(d, wg, &x)) walk(1, item++, x);
    }
    return 0;
}
"""

NBI = (1, 2, 3, 8, 16, 31, 32)
WORKGROUPS = (8, 256, 304)


def column_counts(nbi, P):
    """no tail; a tail of one block; a tail whose parts hold three i-blocks or more (as far as nbi has them: one part when P - 1
    blocks are left), and a tail in several parts"""
    out = [128 * P, 128 * P + 1, 128 * (2 * P - 1), 128 * P + 128 * max(1, P // 3)]
    return sorted(set(out))


@pytest.fixture(scope="module")
def walk_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("walk_i8")
    src = d / "walk_main.cpp"
    src.write_text(WALK_MAIN)
    exe = d / "walk_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True)
    return str(exe)


def replay(walk_program, ncols, nbi, P):
    r = subprocess.run([walk_program, str(ncols), str(nbi), str(P)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    head = [int(x) for x in lines[0].split()]
    bounds = [int(x) for x in lines[1].split()]
    rows = [tuple(int(x) for x in ln.split()) for ln in lines[2:] if ln]
    return head, bounds, rows


@pytest.mark.parametrize("P", WORKGROUPS)
@pytest.mark.parametrize("nbi", NBI)
def test_walks_cover_every_pair_once_in_groups_of_one_or_two(walk_program, nbi, P):
    long_parts = False
    for ncols in column_counts(nbi, P):
        (ncb, nfull, npairs, park, slot), bounds, rows = replay(walk_program, ncols, nbi, P)
        assert ncb == -(-ncols // 128) and nfull == ncb // P * P and npairs == -(-nbi // 2)
        assert slot == 14 * 512 * 128 and park == 2 * slot              # a workgroup parks the residues of two i-blocks
        seen = set()
        items = {}
        for kind, item, cb, lo0, hi0, lo1, hi1, group, sl, ib, tiles in rows:
            assert (cb, ib) not in seen
            seen.add((cb, ib))
            assert 0 <= ib < nbi and sl in (0, 1) and group >= 0
            items.setdefault((kind, item, cb, lo0, hi0, lo1, hi1), []).append((group, sl, ib, tiles))
        assert seen == {(cb, ib) for cb in range(ncb) for ib in range(nbi)}
        tiles_of_block = {}
        for (kind, item, cb, lo0, hi0, lo1, hi1), w in items.items():
            groups = {}
            for k, (group, sl, ib, tiles) in enumerate(w):
                assert group == k // 2 and sl == k % 2                  # in walk order: consecutive twos, slots 0 then 1
                groups.setdefault(group, []).append((sl, ib, tiles))
            assert sorted(groups) == list(range(len(groups)))
            for group, es in groups.items():
                assert len(es) in (1, 2)
                assert [sl for sl, _, _ in es] == list(range(len(es)))  # slots distinct, 0 or 1
                assert all(t == sum(ib + 1 for _, ib, _ in es) for _, _, t in es)
            got = [[ib for _, ib, _ in groups[g]] for g in sorted(groups)]
            assert got == gpu_cases.walk_groups(lo0, hi0, lo1, hi1)     # (the restatement the GPU test uses)
            if kind == 0:
                q = lo1
                assert cb < nfull and (lo0, hi0) == (nbi - 1 - q, nbi - q)
                assert got == ([[nbi - 1 - q, q]] if q < nbi - 1 - q else [[q]])        # one group, in this order
                tiles_of_block.setdefault(cb, set()).add((len(got[0]), groups[0][0][2]))
            else:
                assert cb >= nfull and hi1 <= lo1
                n = hi0 - lo0
                assert got == [list(range(hi0 - 1 - 2 * g, max(hi0 - 3 - 2 * g, lo0 - 1), -1)) for g in range((n + 1) // 2)]
                long_parts = long_parts or n >= 3
        # the items of a block that hold a pair run the same tiles per modulus, nbi + 1, whatever q: they stay in one plane of the
        # block's image; only the lone middle i-block of an odd nbi is shorter
        for cb, kinds in tiles_of_block.items():
            assert {t for n, t in kinds if n == 2} <= {nbi + 1}
            assert {t for n, t in kinds if n == 1} <= {nbi // 2 + 1}
            assert len(kinds) == (1 if nbi % 2 == 0 or nbi == 1 else 2)
        # the restated plan of the GPU test agrees with the header
        want = gpu_cases.plan(ncols, nbi, P)
        assert (want["ncb"], want["nfull"]) == (ncb, nfull)
        assert want["parts"] == ([bounds[q + 1] - bounds[q] for q in range(len(bounds) - 1)] if ncb > nfull else [])
    assert long_parts or nbi < 3, "no tail part with three i-blocks or more among the column counts"


def test_the_gpu_cases_on_256_workgroups():
    """the shapes of tests/test_var_int8_modouter_gpu.py on the device they were chosen for"""
    parts = gpu_cases.plan(12800, 8, 256)["parts"] + gpu_cases.plan(8900, 8, 256)["parts"]
    assert any(n % 2 == 1 and n >= 3 for n in parts) and any(n % 2 == 0 and n >= 4 for n in parts), parts
