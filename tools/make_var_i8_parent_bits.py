"""Write tests/golden/var_i8_parent_bits.npz: what k_var_i8 computes for the seeded cases of tests/test_var_int8_feed.py — per N
var[:129], var[-256:] and the SHA-256 of all 33 000 values.  Run it on a GPU with a build of the commit whose bits are to be kept
(GPT_HIP_LIB selects a library other than the package's own); the test then holds every later kernel to them.
usage: python tools/make_var_i8_parent_bits.py [OUT.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_var_int8_feed as t  # noqa: E402

out = {}
for N in t.SIZES:
    v = t.variances(N, batches=(t.M_ALL,))[0][t.M_ALL]
    out[f"head_{N}"] = v[:t.HEAD].copy()
    out[f"tail_{N}"] = v[-t.TAIL:].copy()
    out[f"sha256_{N}"] = np.array(t.digest(v))
    print(N, out[f"sha256_{N}"], float(v.min()), float(v.max()))
path = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
os.makedirs(os.path.dirname(path), exist_ok=True)
np.savez(path, **out)
print("wrote", path)
