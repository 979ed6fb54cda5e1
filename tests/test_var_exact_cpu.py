"""The exact operand designs of tests/var_exact_designs.py on the CPU (no GPU): every design meets the exactness conditions
of the kernel it is meant for, the numpy restatement of the residue path (tests/var_int8_restatement.py) returns each design's
exact variance inside the bound that tests/test_var_exact.py holds the device to (its docstring has the derivation), and the
designs with all sources on one site drive the leading mixed-radix digit d_13 of the reconstruction."""
import numpy as np
import pytest

from tests import var_exact_designs as vx
from tests import var_int8_restatement as r8


def padded(N):
    return -(-N // 512) * 512


def designs(N):
    p = r8.bits(padded(N))
    return [vx.f1(N), vx.f2(N, 1), vx.f2(N, 7), vx.f2(N, 7, interleaved=True), vx.f2(N, -(-N // 8), offsets=(0, 1, 2)),
            vx.f2(N, -(-N // 8), interleaved=True, offsets=(0, 1, 2)), vx.f2(N, 1, top_bits=p), vx.f2(N, 5, interleaved=True, top_bits=p)]


CASES = [(N, i) for N in (512, 1300, 2048) for i in range(8)] + [(512, "D1"), (512, "D2")]


@pytest.fixture(scope="module")
def cache():
    return {}


def design(cache, N, which):
    if (N, which) not in cache:
        cache[N, which] = vx.f1(N, D=int(which[1])) if isinstance(which, str) else designs(N)[which]
    return cache[N, which]


@pytest.mark.parametrize("N,which", CASES)
def test_designs_meet_their_exactness_conditions(cache, N, which):
    d = design(cache, N, which)
    NP = padded(N)
    d.check_i8(NP, r8.bits(NP))
    assert d.X.shape == (N, d.D) and d.X.min() >= vx.SPACING and d.X.max() < 2 ** 24
    # sites are 1024 or more apart, and so is the origin from every site
    assert len({tuple(x) for x in d.coords.tolist()}) == d.n_sites
    W = d.W()
    assert not np.triu(W, 1).any() and np.all(W[np.tril_indices(N)] != 0)
    if d.plain:
        want = d.expected(np.float64)                        # asserts the fp64 conditions
        assert want[-1] == 1.0 + 2.0 ** -6 and np.all(want[d.n_occupied:] == want[-1]) and np.all(want[:d.n_occupied] < want[-1])
        assert np.all(want > 0.75)
        if which == 0 or isinstance(which, str) or which in (4, 5):      # F1 and the clusters of at most 8: fp32 too
            assert np.bincount(d.site).max() <= 8
            w32 = d.expected(np.float32)
            assert np.array_equal(w32.astype(np.float64), want), "the fp32 reference is the same number"
            assert np.array_equal(W.astype(np.float32).astype(np.float64), W)
    else:
        assert which in (6, 7)


def columns(d):
    """the sites whose queries go through the restatement: all of a clustered design, 160 of F1's, the empty ones, the origin"""
    occ = np.arange(d.n_occupied)
    if d.n_occupied > 200:
        occ = np.unique(np.r_[0:40, d.n_occupied - 40:d.n_occupied, np.arange(0, d.n_occupied, max(d.n_occupied // 80, 1))])
    return np.r_[occ, d.n_occupied:d.n_sites, vx.ORIGIN]


@pytest.mark.parametrize("N,which", CASES)
def test_restatement_meets_the_residue_bound(cache, N, which):
    d = design(cache, N, which)
    NP = padded(N)
    qs = columns(d)
    got = r8.variance(d.W(), d.kstar(qs), vx.C, vx.NOISE, NP)
    ratio, m = vx.i8_error_over_bound(d, NP // 512, qs, got)
    if d.plain:
        equal = int(np.sum(got == d.expected(np.float64)[qs]))
        print(f"{d.name}: worst error / bound {ratio:.3f} (site {qs[m]}), {equal} of {qs.size} columns bit-equal to the exact value")
    else:
        print(f"{d.name}: worst error / bound {ratio:.3f} (site {qs[m]})")
    assert ratio <= 1.0
    assert np.all(got[-1 - (d.n_sites - d.n_occupied):] == 1.0 + 2.0 ** -6)


@pytest.mark.parametrize("N", [512, 1300, 2048])
@pytest.mark.parametrize("top", [False, True])
def test_one_site_designs_drive_the_leading_digit(cache, N, top):
    """All N sources on one site: C[i] = +-(i + 1) 2^(2p) (times 1 - 2^-p in the `top` rows).  d_13 = C / (m_0 .. m_12) to
    the nearest integer, so rows near i = N reach N 4^p 199 / M: 0.894 x 99.5 = 89 at NP = N = 512 and 2048, where +-80 is
    asserted.  N = 1300 is padded to 1536 rows, p is that of 2048 and the product stops at 1300 / 2048 of the range: the reach is
    56.5, and what is asserted at every size is that d_13 comes within 5 % and one digit of its reach, 0.95 reach - 1, on both
    signs (the last rows alternate in sign and exponent, so the extreme row need not be the last one)."""
    d = design(cache, N, 6 if top else 1)
    NP = padded(N)
    p = r8.bits(NP)
    A, _ = r8.quantise_rows(d.W(), p)
    B, _ = r8.quantise_columns(d.kstar(np.array([0])), p, vx.C)
    assert np.abs(A).max() == 2 ** p and np.all(B == 2 ** p)
    if top:
        assert np.all(np.abs(A[4::5][np.tril(np.ones((N, N), bool))[4::5]]) == 2 ** p - 1)
    Csum = r8.plane_sums(r8.planes(A), r8.planes(B))
    dig = r8.garner_digits([r8.balanced(c.astype(np.int64), m) for c, m in zip(Csum, r8.MODULI)])
    d13 = dig[13][:, 0]
    reach = N * 4 ** p * r8.MODULI[13] / r8.modulus_product()
    print(f"{d.name}: d_13 in {d13.min()}..{d13.max()}, N 4^p 199 / M = {reach:.1f}")
    assert d13.max() >= 0.95 * reach - 1 and d13.min() <= -(0.95 * reach - 1)
    if N == NP:
        assert d13.max() >= 80 and d13.min() <= -80
    want = np.array([int(a) for a in A.astype(object).sum(axis=1)], dtype=object) * (1 << p)
    assert np.all(r8.horner_exact(dig)[:, 0] == want)
