"""k_var_i8 after the rework of its operand feed (explicit B-fragment ring, four-deep A ring turned back between the sweeps, chunk
pieces three deep): the integer sums are exact and no fp64 summation order changed, so every output equals, bit for bit, what
the kernel computed before the rework.

Fixture: tests/golden/var_i8_parent_bits.npz, written by tools/make_var_i8_parent_bits.py from a build of the commit BEFORE the
rework (GPT_VAR_INT8=1): per N in {400, 1000, 1300} var[:129], var[-256:] and the SHA-256 of all 33 000 values' bytes.
  N = 400   NP = 512: the diagonal tile only — the A ring wraps from one modulus into the next (and the one after) every tile, and
            the waves that run 2 or 6 steps turn it every time
  N = 1000  NP = 1024: one full tile, then the diagonal: the first hand-over from the straight-line block
  N = 1300  NP = 1536: two full tiles: the straight-line block hands over to itself
M = 33 000 is one whole round on 256 CUs plus a divided tail; M = 1 and 129 must reproduce the same prefix.

Independent of the fixture, the same outputs stay inside an elementwise bound against the fp64 kernel (GPT_VAR_INT8=0) of the
same handle.  The bound is tests/var_int8_bound.py's, carried from "device against restatement" to "device against k_var" through
the exact product V = W k* of the handle's own W and the oracle's k* (u = 2^-53, gamma_k = k u / (1 - k u)):
  residue kernel against restatement   dV1_i = 2^(e_i + f - 2p) sum_k |A'_ik| (delta_k + cross_k) + 40 u |V_i|       (bound.py 2.)
  restatement against exact            dV2_i = 2^(-p-1) (2^f sum_k |W_ik| + 2^e_i sum_k k_k) + N 2^(e_i+f-2p-2) + gamma_26 |V_i|  (bound.py 1.)
  k_var against exact                  dV3_i = (max_k eps_k + gamma_(N+2)) sum_k |W_ik| k_k: its k* is the generating code the residue
                                       kernel shares (relative error eps against the oracle's, bound.py 2a), its dot product of
                                       N terms is an fp64 sum in some order
so the two V differ by at most dV = dV1 + dV2 + dV3 per element, each within dV of the exact one, and
  |var_i8 - var_64| <= sum_i (2 (|V_i| + dV_i) dV_i + dV_i^2) + 2 gamma_(N+1) sum_i (|V_i| + dV_i)^2 + 4 u (c + noise):
both kernels add N squares in a tree and subtract once; the clamp at 0 is 1-Lipschitz.  |V| itself is taken from an fp64 product,
widened by its own gamma_N sum_k |W_ik| k_k.  The bound costs three N x N x M products on the host, so it is evaluated at the
columns COLS: the first 129 (all of the two short calls), the last 256 (the divided tail) and every fourth in between."""
import hashlib
import os

import numpy as np
import pytest

from oracle import gp_oracle as orc
from tests import var_int8_bound as vb
from tests import var_int8_restatement as r8

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "var_i8_parent_bits.npz")
SIZES = (400, 1000, 1300)
M_ALL = 33000
HEAD, TAIL = 129, 256
COLS = np.unique(np.r_[0:HEAD, HEAD:M_ALL - TAIL:4, M_ALL - TAIL:M_ALL])
C0, LS, NOISE, JIT = 0.1, np.array([0.1, 0.1, 0.1]), 1e-4, 1e-10          # tests/test_var_int8_gpu.py


def padded(N):
    return -(-N // 512) * 512


def variances(N, batches=(M_ALL, 1, HEAD)):
    """{M: var of the first M queries by the residue kernel}, the fp64 kernel's var of all M_ALL, the handle's W, X and Xq"""
    from gaussian_process_transportation_amd import _lib
    X, Y, Xq = orc.synthetic_problem(N, M_ALL)
    h = _lib.Handle(0)
    old = os.environ.get("GPT_VAR_INT8")
    try:
        h.fit(X, Y, LS, C0, NOISE, JIT)
        assert h.info()[3] == padded(N)
        W = h.export_inverse_factor()
        os.environ["GPT_VAR_INT8"] = "1"
        out = {}
        for M in batches:
            out[M] = h.predict_all(Xq[:M], var=True)["var"]
            assert h.var_path() == 1, "the residue kernel did not take this launch"
        os.environ["GPT_VAR_INT8"] = "0"
        v64 = h.predict_all(Xq, var=True)["var"]
        assert h.var_path() == 0
    finally:
        if old is None:
            os.environ.pop("GPT_VAR_INT8", None)
        else:
            os.environ["GPT_VAR_INT8"] = old
        h.close()
    return out, v64, W, X, Xq


def digest(v):
    return hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest()


def fp64_path_bound(W, X, Xq, NP, chunk=4096):
    """(M,): the bound of the module docstring on |var of k_var_i8 - var of k_var|"""
    U = vb.U
    N = W.shape[0]
    p = r8.bits(NP)
    A, e = r8.quantise_rows(W, p)
    absA, absW = np.abs(A).astype(np.float64), np.abs(W)
    f = int(r8.exponent(C0))
    rows = np.sum(absW, axis=1)[:, None]
    scale = np.ldexp(1.0, e + f - 2 * p)[:, None]
    out = np.empty(Xq.shape[0])
    for m0 in range(0, Xq.shape[0], chunk):
        q = Xq[m0:m0 + chunk]
        Kst = orc.kernel_cross(q, X, C0, LS).T.copy()
        eps = vb.kernel_rel_error(X, q, LS, C0, "rbf")
        WK = absW @ Kst
        Vabs = np.abs(W @ Kst) + vb.gamma(N) * WK
        x = np.ldexp(Kst, p - f)
        delta = eps * x
        dB = delta + (np.abs(x - np.floor(x) - 0.5) <= delta)
        dV1 = scale * (absA @ dB) + 40 * U * Vabs
        dV2 = (2.0 ** (-p - 1) * (2.0 ** f * rows + np.ldexp(1.0, e)[:, None] * np.sum(Kst, axis=0)[None, :]) + N * scale / 4
               + vb.gamma(26) * Vabs)
        dV3 = (np.max(eps, axis=0)[None, :] + vb.gamma(N + 2)) * WK
        dV = dV1 + dV2 + dV3
        hi = Vabs + dV
        out[m0:m0 + chunk] = (np.sum(2 * hi * dV + dV * dV, axis=0) + 2 * vb.gamma(N + 1) * np.sum(hi * hi, axis=0)
                              + 4 * U * (C0 + NOISE))
    return out * (1 + 1e-9)               # (the bound itself is computed in fp64)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module", params=SIZES, ids=[f"N{n}" for n in SIZES])
def case(request):
    """every launch of one size, made once and shared by the two tests"""
    N = request.param
    out, v64, W, X, Xq = variances(N)
    return dict(N=N, out=out, v64=v64, W=W, X=X, Xq=Xq)


def test_bits_of_the_parent_build(case, golden):
    N, v = case["N"], case["out"][M_ALL]
    assert v.shape == (M_ALL,)
    assert np.array_equal(v[:HEAD], golden[f"head_{N}"])
    assert np.array_equal(v[-TAIL:], golden[f"tail_{N}"])
    assert digest(v) == str(golden[f"sha256_{N}"])
    assert np.array_equal(case["out"][1], golden[f"head_{N}"][:1])
    assert np.array_equal(case["out"][HEAD], golden[f"head_{N}"])


def test_inside_the_derived_bound_of_the_fp64_kernel(case):
    N = case["N"]
    bound = fp64_path_bound(case["W"], case["X"], case["Xq"][COLS], padded(N))
    worst = 0.0
    for M, v in case["out"].items():
        cols = COLS[COLS < M]
        err = np.abs(v[cols] - case["v64"][cols])
        worst = max(worst, float(np.max(err / bound[:cols.size])))
        print(f"N = {N}, M = {M}: max |var_i8 - var_64| = {err.max():.3e}, worst error / bound {np.max(err / bound[:cols.size]):.3g}")
        assert np.all(err <= bound[:cols.size])
    print(f"N = {N}: the bound is at most {bound.max():.2e} ({bound.max() / C0:.2e} c), worst error / bound {worst:.3g}")
    assert bound.max() < 1e-11            # (and it is no looser than the fixed figure tests/test_var_int8_gpu.py holds the two paths to)
