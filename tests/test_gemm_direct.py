"""The fp64 MFMA GEMM (k_gemm in csrc/gpt_fit.hip) on its own, through the test hook gpt_debug_dgemm: all nine
instantiations (layouts A B, A^T B, A B^T x tile edges 32, 64, 128) and lower_only at the three edges, against numpy.

Exact cases: operands hold integers in [-8, 8] and alpha is one of 1, -1, -0.5, 2.  Every product is an integer of at most 64
and every partial sum, in any order, an integer of at most 64 K <= 2^18 for K <= 4096: all are exactly representable, so every
summation order gives the same fp64 number, numpy's A @ B is THE answer and the device must return it bit for bit.
C is pre-filled with a sentinel and embedded, like the operands, in a wider array: nothing outside the M x N window may
change, and with lower_only an element above the diagonal is either untouched or the exact product (the kernel skips by tile
and by wave quadrant, so parts of the upper triangle of diagonal tiles are written)."""
import numpy as np
import pytest

LAYOUTS = ("AB", "AT", "BT")
EDGES = (32, 64, 128)
SENTINEL = -12345.678
# (layout, edge) and ("lower", edge) pairs that an exact case has hit and passed; checked by the last test of the file
COVERED = set()

# launch_gemm's rule (csrc/gpt_fit.hip: gemm_tile_edge), restated for the expected edges below:
# tiles = ceil(M / 128) ceil(N / 128), halved for lower_only; edge 32 below 256 tiles, 64 below 2500, 128 from there on.


def _expected_edge(M, N, lower):
    tiles = -(-M // 128) * -(-N // 128) * (0.5 if lower else 1.0)
    return 32 if tiles < 256 else (64 if tiles < 2500 else 128)


# M, N, K, lower_only, alpha, (extra lda, ldb, ldc).  Every shape is run in each of the three layouts.
EXACT_SHAPES = [
    # edge 32: odd and even multiples of 64, K from two chunks up to 4096
    (64, 64, 64, False, 1.0, (0, 0, 0)),
    (64, 64, 64, True, -1.0, (6, 2, 10)),            # lower_only, the smallest product: 2 x 2 tiles of 32, folded
    (192, 64, 4096, False, -0.5, (2, 4, 6)),         # thin
    (64, 1088, 192, False, 2.0, (0, 8, 2)),          # wide
    (1088, 192, 512, False, -1.0, (10, 0, 4)),
    (512, 512, 1088, False, 1.0, (0, 0, 0)),
    (192, 192, 512, True, 2.0, (4, 4, 4)),           # lower_only, 6 tile rows of 32
    (1088, 1088, 64, True, -0.5, (0, 2, 0)),         # lower_only, 34 tile rows
    (1600, 1600, 64, True, 1.0, (2, 0, 2)),          # lower_only, 50 tile rows
    (1024, 64, 1024, False, 1.0, (0, 0, 0)),         # the surface SVGP's NP x BP x NP, one batch column block
    (512, 1024, 512, False, 1.0, (0, 0, 0)),         # NP x BP x NP at BP = 1024
    (1024, 1024, 64, True, -0.5, (0, 0, 0)),         # NP x NP x BP, lower (-1/2 Abar A^T)
    # edge 64: from 256 tiles on
    (2048, 2048, 64, False, 1.0, (0, 0, 0)),         # 256 tiles: the first shape at edge 64
    (2112, 2112, 192, False, -1.0, (2, 2, 2)),       # 33 tile rows (odd multiple of 64)
    (2048, 1024, 2048, False, 1.0, (0, 0, 0)),       # 128 tiles: edge 32 still (NP = 2048, BP = 1024)
    (4096, 1024, 256, False, 2.0, (0, 0, 0)),        # 256 tiles, thin for its height: edge 64, M != N
    (1024, 4160, 128, False, -0.5, (4, 0, 2)),       # wide at edge 64
    (2944, 2944, 64, True, 1.0, (0, 0, 0)),          # lower_only: 23 x 23 / 2 = 264.5 tiles, edge 64, 46 tile rows (even)
    (3008, 3008, 64, True, -1.0, (2, 2, 2)),         # 47 tile rows of 64: the fold's middle row
    (2048, 2048, 1024, False, 1.0, (0, 0, 0)),       # NP x NP x BP, full
    # edge 128: from 2500 tiles on
    (6400, 6400, 64, False, 1.0, (0, 0, 0)),         # exactly 2500 whole tiles
    (6464, 6464, 64, False, -0.5, (2, 4, 6)),        # 51 x 51 tiles, the last row and column half empty: the guarded partial tiles
    (9088, 9088, 64, True, 1.0, (0, 0, 0)),          # lower_only: 71 x 71 / 2 = 2520.5 tiles; 71 whole tile rows (the fold's middle row)
    (9152, 9152, 64, True, 2.0, (0, 0, 2)),          # lower_only, 72 tile rows (even fold), the last one half empty
    (12800, 3200, 128, False, -1.0, (0, 0, 0)),      # 100 x 25 tiles: M != N at edge 128
]


def _ids(shape):
    M, N, K, lower, alpha, pad = shape
    return f"{M}x{N}x{K}{'_lower' if lower else ''}_a{alpha:g}_ld{pad[0]}.{pad[1]}.{pad[2]}"


def _embed(rng, rows, cols, extra, fill):
    """(rows, cols) drawn by `fill` in the top-left of a (rows, cols + extra) array whose other columns hold finite junk:
    reading past the row length would change the product."""
    a = np.full((rows, cols + extra), 3.0)
    a[:, :cols] = fill(rng, (rows, cols))
    return a


def _ints(rng, shape):
    return rng.integers(-8, 9, shape).astype(np.float64)


def _normal(rng, shape):
    return rng.standard_normal(shape)


def _operands(rng, layout, M, N, K, pad, fill):
    """Stored operands (with their row padding) and op(A), op(B) as views for the reference."""
    A = _embed(rng, K if layout == "AT" else M, M if layout == "AT" else K, pad[0], fill)
    B = _embed(rng, N if layout == "BT" else K, K if layout == "BT" else N, pad[1], fill)
    opA = A[:, :M].T if layout == "AT" else A[:, :K]
    opB = B[:, :K].T if layout == "BT" else B[:, :N]
    return A, B, opA, opB


def _run(layout, M, N, K, alpha, lower, A, B, ldc_extra):
    from gaussian_process_transportation_amd import _lib
    out = np.full((M, N + ldc_extra), SENTINEL)
    edge = _lib.debug_dgemm(A, B, out, M, N, K, alpha=alpha, at=layout == "AT", bt=layout == "BT", lower_only=lower)
    return out, edge


def _wrong_pattern(bad, edge):
    """Where the wrong elements are, for the failure message: counts, the bounding box and the tiles touched."""
    i, j = np.nonzero(bad)
    tiles = sorted(set(zip((i // edge).tolist(), (j // edge).tolist())))
    return (f"{bad.sum()} wrong elements, rows {i.min()}..{i.max()}, columns {j.min()}..{j.max()}, "
            f"{len(tiles)} tiles of {edge}, first {tiles[:6]}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_ids)
def test_exact_integer_products_are_bit_identical(shape, layout):
    M, N, K, lower, alpha, pad = shape
    assert K <= 4096 and alpha in (1.0, -1.0, -0.5, 2.0)
    rng = np.random.default_rng([M, N, K, LAYOUTS.index(layout)])
    A, B, opA, opB = _operands(rng, layout, M, N, K, pad, _ints)
    out, edge = _run(layout, M, N, K, alpha, lower, A, B, pad[2])
    assert edge == _expected_edge(M, N, lower), f"tile edge {edge}"
    ref = alpha * (opA @ opB)
    assert np.all(ref == np.rint(2 * ref) / 2) and np.abs(ref).max() <= 2 * 64 * K      # integers (halves with alpha = -0.5)
    win = out[:, :N]
    assert np.all(out[:, N:] == SENTINEL), "written right of the M x N window: " + _wrong_pattern(
        np.pad(out[:, N:] != SENTINEL, ((0, 0), (N, 0))), edge)
    if lower:
        tri = np.tril(np.ones((M, N), bool))
        bad = np.where(tri, win != ref, (win != ref) & (win != SENTINEL))
    else:
        bad = win != ref
    assert not bad.any(), f"{layout} edge {edge}: " + _wrong_pattern(bad, edge)
    COVERED.add((layout, edge))
    if lower:
        COVERED.add(("lower", edge))


# One real-valued case per (layout, edge).  Standard normal operands; for any order of summation
# |fl(sum_k a_k b_k) - sum_k a_k b_k| <= gamma_K sum_k |a_k b_k|, gamma_K = K u / (1 - K u), u = 2^-53 (Higham, Accuracy and
# Stability of Numerical Algorithms, section 3.1; a fused multiply-add only lowers it).  The numpy reference carries the same
# error, so the two may differ by twice that: 2 K u (|A| |B|)_ij, elementwise (K u <= 2^-41: the 1 - K u is far below the
# slack of bounding both sides by the full K).  Derived, not measured.
REAL_SHAPES = {32: (320, 192, 1088), 64: (2112, 2048, 320), 128: (6464, 6400, 128)}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("edge", EDGES)
def test_real_operands_within_the_summation_bound(edge, layout):
    M, N, K = REAL_SHAPES[edge]
    rng = np.random.default_rng([edge, LAYOUTS.index(layout)])
    A, B, opA, opB = _operands(rng, layout, M, N, K, (2, 2, 2), _normal)
    out, got_edge = _run(layout, M, N, K, 1.0, False, A, B, 2)
    assert got_edge == edge
    ref = opA @ opB
    bound = 2 * K * 2.0 ** -53 * (np.abs(opA) @ np.abs(opB))
    err = np.abs(out[:, :N] - ref)
    print(f"{layout} edge {edge} {M}x{N}x{K}: worst error / bound {np.max(err / bound):.3f}")
    assert np.all(out[:, N:] == SENTINEL)
    assert np.all(err <= bound), _wrong_pattern(err > bound, edge)


def test_contract_violations_are_refused():
    """The argument checks come before the first HIP call: no GPU needed."""
    from gaussian_process_transportation_amd import _lib
    A = np.zeros((128, 128))
    out = np.zeros((128, 128))
    for kw in (dict(M=96, N=64, K=64), dict(M=64, N=64, K=32), dict(M=64, N=128, K=64, lower_only=True),
               dict(M=64, N=64, K=64, at=True, bt=True), dict(M=0, N=64, K=64)):
        with pytest.raises(ValueError):
            _lib.debug_dgemm(A, A, out, **kw)
    with pytest.raises(ValueError, match="leading dimension"):
        _lib.debug_dgemm(np.zeros((64, 66)), np.zeros((64, 62)), out, 64, 64, 64)        # ldb below the row length
    with pytest.raises(ValueError, match="leading dimension"):
        _lib.debug_dgemm(np.zeros((64, 65)), A, out, 64, 64, 64)                         # odd lda
    assert not out.any()


# With the default thresholds a lower_only product never has a single tile: M = 64 picks edge 32 (2 x 2 tiles, folded).  The
# unfolded TM == TN == 1 grid is what GPT_GEMM_TS32_BELOW=0 (the launcher's A/B knob, read once per process) gives for
# M = N = 64 at edge 64, so that case runs in a child process of its own.
_SINGLE_TILE_CHILD = """
import numpy as np
from tests import test_gemm_direct as t
for layout in t.LAYOUTS:
    rng = np.random.default_rng(7)
    A, B, opA, opB = t._operands(rng, layout, 64, 64, 64, (2, 4, 6), t._ints)
    out, edge = t._run(layout, 64, 64, 64, -1.0, True, A, B, 6)
    assert edge == 64, edge
    ref = -(opA @ opB)
    win = out[:, :64]
    tri = np.tril(np.ones((64, 64), bool))
    assert np.all(out[:, 64:] == t.SENTINEL)
    assert np.array_equal(win[tri], ref[tri]), layout
    assert np.all((win == ref) | (win == t.SENTINEL)), layout
print("single tile ok")
"""


@pytest.mark.gpu
def test_lower_only_single_tile_is_not_folded():
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    env = dict(os.environ, GPT_GEMM_TS32_BELOW="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _SINGLE_TILE_CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "single tile ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_every_instantiation_was_covered_by_an_exact_case():
    """Runs after the exact cases (file order): all nine (layout, edge) pairs and lower_only at the three edges must
    have been hit, as reported by the launcher itself, and passed."""
    want = {(layout, e) for layout in LAYOUTS for e in EDGES} | {("lower", e) for e in EDGES}
    print("covered:", sorted(COVERED, key=str))
    assert want <= COVERED, f"not covered: {sorted(want - COVERED, key=str)}"
