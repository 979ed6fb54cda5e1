"""The work split of k_var_i8 into items (csrc/gpt_plan_i8.h): whole groups of P column blocks are dealt as (column block, i-block
pair) items, var_i8_group_item; what is left goes to the tail's parts, var_i8_tail_item, as before.  A small program of its own
replays both on the CPU, as tests/test_var_int8_cpu.py does for the tail.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc")

# one line per item: kind (0 group item, 1 tail part), round, item step, workgroup, block, image, lo0 hi0 lo1 hi1
ITEMS_MAIN = r"""
#include "gpt_plan_i8.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    const long long ncols = atoll(argv[1]);
    const int nbi = atoi(argv[2]), P = atoi(argv[3]);
    gpt::VarI8PlanDev d = gpt::build_var_i8_plan(ncols, nbi, P);
    const int npairs = gpt::var_i8_npairs(nbi);
    printf("%lld %lld %d\n", (long long)d.ncb, (long long)d.nfull, npairs);
    for (long long r = 0; r < d.nfull / P; ++r) {
        d.rnd_begin = r; d.rnd_end = r + 1;               // one round per launch: the images are those of this round
        for (int k = 0; k < npairs; ++k)
            for (int wg = 0; wg < P; ++wg) {
                const gpt::VarI8Item x = gpt::var_i8_group_item(d, r, k, wg);
                printf("0 %lld %d %d %lld %lld %d %d %d %d\n", r, k, wg, (long long)x.cb, (long long)x.img, x.lo[0], x.hi[0], x.lo[1], x.hi[1]);
            }
    }
    d.rnd_begin = d.rnd_end = d.nfull / P;
    for (int wg = 0; wg < P; ++wg) {
        gpt::VarI8Item x;
        if (gpt::var_i8_tail_as_item(d, wg, &x))
            printf("1 -1 -1 %d %lld %lld %d %d %d %d\n", wg, (long long)x.cb, (long long)x.img, x.lo[0], x.hi[0], x.lo[1], x.hi[1]);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def items_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("items_i8")
    src = d / "items_main.cpp"
    src.write_text(ITEMS_MAIN)
    exe = d / "items_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("ncols,nbi,P", [(33000, 4, 256), (500000, 16, 256), (33000, 16, 256), (70000, 32, 256), (33000, 3, 256),
                                         (300, 1, 256), (40000, 5, 24), (129, 2, 256)])
def test_items_and_tail_parts_cover_every_pair_once(items_program, ncols, nbi, P):
    out = subprocess.run([items_program, str(ncols), str(nbi), str(P)], check=True, capture_output=True, text=True).stdout.split("\n")
    ncb, nfull, npairs = (int(x) for x in out[0].split())
    assert ncb == -(-ncols // 128) and nfull == ncb // P * P and npairs == -(-nbi // 2)
    seen = set()
    q_of_wg = {}
    n_items = 0
    for line in out[1:]:
        if not line:
            continue
        kind, rnd, step, wg, cb, img, lo0, hi0, lo1, hi1 = (int(x) for x in line.split())
        assert 0 <= img < P                                   # the image buffer holds one group
        ranges = [(lo0, hi0)] + ([(lo1, hi1)] if hi1 > lo1 else [])
        if kind == 0:
            n_items += 1
            assert rnd * P <= cb < (rnd + 1) * P and cb < nfull and img == cb - rnd * P
            q = lo1
            assert (lo0, hi0) == (nbi - 1 - q, nbi - q) and 0 <= q < npairs
            tiles = sum(ib + 1 for lo, hi in ranges for ib in range(lo, hi))
            if nbi % 2 == 0:
                assert len(ranges) == 2 and tiles == nbi + 1
            else:
                assert tiles == (nbi + 1 if q < nbi // 2 else nbi // 2 + 1)
            if P % npairs == 0:                               # a workgroup keeps its i-blocks for the whole launch
                assert q_of_wg.setdefault(wg, q) == q
        else:
            assert nfull <= cb < ncb and img == cb - nfull and len(ranges) == 1
        for lo, hi in ranges:
            assert 0 <= lo < hi <= nbi
            for ib in range(lo, hi):
                assert (cb, ib) not in seen
                seen.add((cb, ib))
    assert n_items == nfull * npairs
    assert seen == {(cb, ib) for cb in range(ncb) for ib in range(nbi)}
