"""Write tests/golden/var_i8_items_parent_bits.npz: what k_var_i8 computes for the cases of tests/test_var_int8_items_gpu.py, `var` at
the test's sample of queries per case.  Run it on a GPU with a build of the commit whose bits are to be kept (GPT_HIP_LIB selects a
library other than the package's own); the test then holds every later kernel to them.
usage: python tools/make_var_i8_items_parent_bits.py [OUT.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_var_int8_items_gpu as t  # noqa: E402

out = {}
idx = t.sample()
for case in t.CASES:
    var, dt = t.variance(case)
    out["var_" + case["id"]] = var[idx]
    print(f"{case['id']}: fit + predict {dt:.2f} s, var in [{var.min():.6g}, {var.max():.6g}], kept {idx.size} of {var.size}")
path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
os.makedirs(os.path.dirname(path), exist_ok=True)
np.savez(path, **out)
print("wrote", path)
