"""The residue arithmetic of k_var_i8 (csrc/gpt_residue_i8.h: byte dot products, one fp32 quotient, no fix-up) on the CPU, through a
small g++ program of its own that includes the header without HIP (the dot product falls back to a plain loop).  The program
compares against `%` on 64-bit integers and counts mismatches; a sample of what it computed is printed and checked again here with
Python integers.  No GPU."""
import os
import shutil
import subprocess

import pytest

from tests import var_int8_restatement as r8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_transportation_amd", "csrc")

MAIN = r"""
#include "gpt_residue_i8.h"
#include <cstdio>
#include <cstdlib>
#include <random>
using namespace gpt;
static int balanced(long long x, int m) { long long r = x % m; if (r < 0) r += m; return (int)(r > (m - 1) / 2 ? r - m : r); }
static long long n_checked, n_bad;
static void begin() { n_checked = n_bad = 0; }
static void end(const char* name) { printf("%s %lld %lld\n", name, n_checked, n_bad); }
// operand x: every modulus against %, the integer as well as the stored byte
static void operand(long long x, bool sample) {
    uint32_t lo, hi;
    i8_operand_split((double)x, lo, hi);
    for (int j = 0; j < I8_NMOD; ++j) {
        const uint32_t rb = i8_operand_bits(lo, hi, i8_res_tab(), j);
        const int want = balanced(x, I8_MODULI[j]);
        ++n_checked;
        if (i8_bits_byte(rb) != want || (j > 0 && i8_bits_int(rb) != want)) ++n_bad;
        if (sample) printf("S op %lld %d %d\n", x, I8_MODULI[j], i8_bits_byte(rb));
    }
}
static void accumulator(int a, bool sample) {
    for (int j = 0; j < I8_NMOD; ++j) {
        const uint32_t rb = i8_acc_bits(a, i8_res_tab(), j);
        const int want = balanced(a, I8_MODULI[j]);
        ++n_checked;
        if (i8_bits_byte(rb) != want || (j > 0 && i8_bits_int(rb) != want)) ++n_bad;
        if (sample) printf("S acc %d %d %d\n", a, I8_MODULI[j], i8_bits_byte(rb));
    }
}
int main() {
    const I8ResTab& T = i8_res_tab();
    // 1. every t the dot products can return (t < 2^19 covers both inputs: see the header), every modulus: congruent, balanced
    begin();
    for (int j = 0; j < I8_NMOD; ++j) {
        const int m = I8_MODULI[j];
        for (uint32_t t = 0; t < (1u << 19); ++t) {
            const uint32_t rb = i8_balanced_bits(I8_FBIAS_BITS + t, T.m[j], T.rm[j]);
            const int r = i8_bits_int(rb);
            ++n_checked;
            const bool ok = ((long long)t - r) % m == 0 && (j > 0 ? (r >= -(m - 1) / 2 && r <= (m - 1) / 2) : (r >= -128 && r <= 128))
                            && i8_bits_byte(rb) == balanced(t, m);
            if (!ok) ++n_bad;
        }
    }
    end("quotient");
    // the largest t either input reaches stays below 2^19
    begin();
    for (int j = 0; j < I8_NMOD; ++j) {
        uint32_t lo = T.op_lo[j], hi = T.op_hi[j], top = 0;
        for (int i = 0; i < 4; ++i) top += 255u * ((lo >> (8 * i)) & 255u) + (i < 2 ? 255u : (i == 2 ? 15u : 0u)) * ((hi >> (8 * i)) & 255u);
        top += (T.op_k[j] > T.acc_k[j] ? T.op_k[j] : T.acc_k[j]) - I8_FBIAS_BITS;
        ++n_checked;
        if (top >= (1u << 19) || (hi >> 24) != 0) ++n_bad;
    }
    end("reach");
    // 2. operands
    begin();
    for (long long x = 0; x < (1 << 20); ++x) { operand(x, x % 4099 == 0); operand(-x, x % 4099 == 7); }
    end("operand_small");
    begin();
    for (int k = 0; k <= 50; ++k)
        for (int d = -1; d <= 1; ++d) { const long long x = (1LL << k) + d; operand(x, true); operand(-x, true); }
    end("operand_pow2");
    begin();
    std::mt19937_64 rng(20240607);
    for (int i = 0; i < 1000000; ++i) {
        const unsigned long long u = rng();
        long long x = (long long)(u & ((1ULL << 48) - 1));
        if (i % 8 == 0) x |= (long long)((u >> 48) & 3) << 48;         // up to 2^50: the operands of the smallest models
        operand((u >> 63) ? -x : x, i % 997 == 0);
    }
    end("operand_random");
    // 3. accumulators
    begin();
    const int edges[] = {0, 1, -1, 1 << 28, -(1 << 28), (1 << 28) - 1, -(1 << 28) + 1, 127, 128, -128, -129, 255, 256, 1 << 30, -(1 << 30)};
    for (int a : edges) accumulator(a, true);
    end("acc_edges");
    begin();
    for (int i = 0; i < 1000000; ++i) {
        const unsigned long long u = rng();
        const int a = (int)(u % ((1ULL << 29) + 1)) - (1 << 28);
        accumulator(a, i % 997 == 0);
    }
    end("acc_random");
    return 0;
}
"""

CHECKS = ("quotient", "reach", "operand_small", "operand_pow2", "operand_random", "acc_edges", "acc_random")


@pytest.fixture(scope="module")
def residue_run(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("residue_i8")
    src = d / "residue_main.cpp"
    src.write_text(MAIN)
    exe = d / "residue_main"
    subprocess.run([cxx, "-std=c++17", "-O2", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True)
    assert "runtime error" not in out.stderr
    counts, samples = {}, []
    for line in out.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] == "S":
            samples.append((f[1], int(f[2]), int(f[3]), int(f[4])))
        else:
            counts[f[0]] = (int(f[1]), int(f[2]))
    return counts, samples


def test_header_moduli_are_the_restatements():
    with open(os.path.join(CSRC, "gpt_plan_i8.h")) as fh:
        text = fh.read()
    assert "{" + ", ".join(str(m) for m in r8.MODULI) + "}" in text


@pytest.mark.parametrize("name", CHECKS)
def test_residues_equal_integer_remainders(residue_run, name):
    counts, _ = residue_run
    checked, bad = counts[name]
    expect = {"quotient": 14 << 19, "reach": 14, "operand_small": 2 * 14 << 20, "operand_pow2": 51 * 3 * 2 * 14,
              "operand_random": 14 * 10 ** 6, "acc_edges": 15 * 14, "acc_random": 14 * 10 ** 6}[name]
    print(f"{name}: {checked} checked, {bad} wrong")
    assert checked == expect
    assert bad == 0


def test_sampled_bytes_against_python_integers(residue_run):
    _, samples = residue_run
    assert len(samples) > 3000
    kinds = {k for k, _, _, _ in samples}
    assert kinds == {"op", "acc"}
    assert any(abs(x) == 1 << 50 for k, x, _, _ in samples if k == "op") and any(abs(x) == 1 << 48 for k, x, _, _ in samples if k == "op")
    assert any(abs(x) == 1 << 28 for k, x, _, _ in samples if k == "acc")
    for _, x, m, byte in samples:
        r = x % m
        if r > (m - 1) // 2:
            r -= m
        assert byte == r, (x, m, byte)


# ---- Garner's digits (inv_i folded into the weights): against exact integers
GARNER_MAIN = r"""
#include "gpt_residue_i8.h"
#include <cstdio>
#include <random>
using namespace gpt;
typedef __int128 i128;
static void show(i128 C) {
    float r[I8_NMOD], d[I8_NMOD];
    for (int j = 0; j < I8_NMOD; ++j) {
        const int m = I8_MODULI[j];
        int x = (int)(C % m);
        if (x < 0) x += m;
        r[j] = (float)(x > (m - 1) / 2 ? x - m : x);
    }
    i8_garner_digits(r, d);
    const bool neg = C < 0;
    const unsigned __int128 a = neg ? (unsigned __int128)(-C) : (unsigned __int128)C;
    printf("%s%llx%016llx", neg ? "-" : "", (unsigned long long)(a >> 64), (unsigned long long)a);
    for (int j = 0; j < I8_NMOD; ++j) printf(" %.1f", (double)d[j]);
    printf("\n");
}
int main() {
    i128 M = 1;
    for (int j = 0; j < I8_NMOD; ++j) M *= I8_MODULI[j];
    const i128 half = (M - 1) / 2;                       // |C| <= half: M is even, so this is |C| < M / 2
    for (int c = -300; c <= 300; ++c) show(c);
    for (int np = 8192, p = 48; np <= 16384; np *= 2, --p) { show((i128)np << (2 * p)); show(-((i128)np << (2 * p))); }
    show(half); show(-half); show(half - 1); show(1 - half);
    std::mt19937_64 rng(77);
    for (int i = 0; i < 20000; ++i) {
        const unsigned __int128 u = ((unsigned __int128)rng() << 64) | rng();
        i128 C = (i128)(u % (unsigned __int128)(2 * half + 1)) - half;
        if (i % 4 == 1) C >>= (rng() % 100);             // every magnitude: the leading digits vanish
        show(C);
    }
    return 0;
}
"""


def test_garner_digits_against_exact_integers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "garner_main.cpp"
    src.write_text(GARNER_MAIN)
    exe = tmp_path / "garner_main"
    subprocess.run([cxx, "-std=gnu++17", "-O2", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True)
    assert "runtime error" not in out.stderr
    M = r8.modulus_product()
    lines = [ln.split() for ln in out.stdout.split("\n") if ln]
    assert len(lines) == 601 + 4 + 4 + 20000
    seen = set()
    for f in lines:
        C = int(f[0], 16)
        assert 2 * abs(C) < M
        seen.add(C)
        got = [float(x) for x in f[1:]]
        want, rest = [], C
        for m in r8.MODULI:
            d = rest % m
            if d > (m - 1) // 2:
                d -= m
            want.append(d)
            rest = (rest - d) // m
        assert rest == 0
        assert got == [float(d) for d in want], C
    for NP, p in ((8192, 48), (16384, 47)):
        assert NP << (2 * p) in seen and -(NP << (2 * p)) in seen
    assert (M - 1) // 2 in seen and 0 in seen
