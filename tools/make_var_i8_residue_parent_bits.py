"""Write tests/golden/var_i8_residue_parent_bits.npz: what k_var_i8 computes for the cases of tests/test_var_int8_residue_gpu.py, `var`
in full per case.  Run it on a GPU with a build of the commit whose bits are to be kept (GPT_HIP_LIB selects a library other than
the package's own); the test then holds every later kernel to them.

For the case with c = 2^f and queries copied from sources it also says how many columns reach B' = 2^p: a coincident pair has
h = 0 to well below an ulp of ln c, so its k* is exp_tab(ln c) (csrc/gpt_exp.h), replayed here in exact rational arithmetic, and
B' = rint(k* 2^(p - f)).
usage: python tools/make_var_i8_residue_parent_bits.py [OUT.npz]"""
import math
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_var_int8_residue_gpu as t  # noqa: E402
from tests import var_int8_restatement as r8  # noqa: E402


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def exp_tab_of_log(c):
    """csrc/gpt_exp.h exp_tab at ln c, for a c whose table entry is T[0] = 1 (c a power of two)"""
    inv, hi, lo = (float.fromhex(x) for x in ("0x1.71547652b82fep+8", "0x1.62e42fee00000p-9", "0x1.a39ef35793c76p-41"))
    x = math.log(c)
    n = float(round(x * inv))
    assert int(n) % 256 == 0
    r = fma(n, -lo, fma(n, -hi, x))
    pz = fma(r, 1.0 / 24.0, 1.0 / 6.0)
    for k in (0.5, 1.0, 1.0):
        pz = fma(pz, r, k)
    return math.ldexp(pz, int(n) >> 8)


out = {}
for case in t.CASES:
    var, dt = t.variance(case)
    out["var_" + case["id"]] = var
    print(f"{case['id']}: fit + predict {dt:.2f} s, var in [{var.min():.6g}, {var.max():.6g}]")
    if case["copies"]:
        p = r8.bits(-(-case["N"] // 512) * 512)
        f = int(r8.exponent(case["c"]))
        k0 = exp_tab_of_log(case["c"])
        top = round(math.ldexp(k0, p - f)) == 1 << p
        print(f"  k* of a coincident pair = c (1 + {k0 / case['c'] - 1:.3g}), p = {p}, f = {f}: "
              f"{case['copies'] if top else 0} columns hold an operand B' = 2^p")
path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
os.makedirs(os.path.dirname(path), exist_ok=True)
np.savez(path, **out)
print("wrote", path)
