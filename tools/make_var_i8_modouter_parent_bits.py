"""Write tests/golden/var_i8_modouter_parent_bits.npz: what k_var_i8 computes for the cases of tests/test_var_int8_modouter_gpu.py,
`var` at the test's sample of queries per case.  Run it on a GPU with a build of the commit whose bits are to be kept (GPT_HIP_LIB
selects a library other than the package's own); the test then holds every later kernel to them.  It also prints, for the device's
workgroup count, the i-block counts of the tail parts of every case: the N = 4096 cases have to show an odd count >= 3 and an even
count >= 4 between them (the test asserts it).
usage: python tools/make_var_i8_modouter_parent_bits.py [OUT.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_var_int8_modouter_gpu as t  # noqa: E402

out = {}
P = t.workgroups()
for case in t.CASES:
    var = t.variance(case)
    idx = t.sample(case["M"])
    out["var_" + case["id"]] = var[idx]
    pl = t.plan(case["M"], case["N"] // 512, P)
    print(f"{case['id']}: var in [{var.min():.6g}, {var.max():.6g}], kept {idx.size} of {var.size}; {P} workgroups: "
          f"{pl['nfull']} of {pl['ncb']} blocks in whole groups, i-blocks per tail part {pl['parts']}")
path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
os.makedirs(os.path.dirname(path), exist_ok=True)
np.savez(path, **out)
print("wrote", path)
