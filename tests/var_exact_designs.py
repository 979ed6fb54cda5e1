"""Operands for the variance kernels (k_var, k_var_i8) whose answer is known exactly, and that answer.  Host only: numpy and
Python integers / fractions.  Used by tests/test_var_exact_cpu.py (no GPU) and tests/test_var_exact.py (GPU).

var_m = c + noise - sum_i V[i, m]^2, V = W K*^T.  The kernels generate K* themselves and read W from the fit, so a test can
only choose the sources, the queries and - through gpt_debug_set_inverse_factor - W:

  * c = 1, length-scale 1, noise 2^-6; sources and queries on SITES of an integer lattice with spacing 1024 (coordinates
    1024 .. < 2^24, exact in fp32 too).  A query on a site sees k* = 1 exactly for every source on that site (distance 0: the
    table exp returns T[0] = 1, the Matern prefactor is 1) and exactly 0 for every other source (the exponent is clamped at
    -800, where the exp underflows to 0; the Matern prefactor is bounded), for all four kernel types.  So
    V[i, m] = sum of W[i, k] over the sources k <= i on the site of query m: a sum of chosen numbers.
  * F1 (one-hot): every source has its own site, V[i, m] = W[i, k(m)], var = 1 + 2^-6 - sum_{i >= k} W[i, k]^2 with
    W[i, k] = w 2^E, w a random non-zero integer in [-8, 8]: with one query per source every element of W has a column that
    changes when the element is dropped, counted twice or read from another place.
  * F2 (clusters): the sources share G sites, in contiguous ranges or interleaved (k mod G); rows are saturated,
    W[i, k] = s 2^(E_i) for all k <= i with s = +1, -1 or alternating in k, E_i one of a few exponents.  G = 1 puts all N
    sources on one site: V[i] = +-(i + 1) 2^(E_i), and the integer product of the residue path reaches (i + 1) 2^(2p), up to
    N 2^(2p) - its leading mixed-radix digits are in use.  `top` (residue path only) gives some rows (1 - 2^-p) 2^(E_i),
    i.e. A' = 2^p - 1: every residue plane of those rows is busy.
  * "exactly 1" needs a distance of exactly 0.  The kernels form x / (l sqrt 2) - q / (l sqrt 2) from products that are each
    rounded, and the compiler may fuse one product into the subtraction: a coincident pair then gives the rounding error of
    x / sqrt 2, of the order |x| u, not 0.  RBF does not see it (exp(-h), h ~ u^2), but Matern 1/2 is 1 - r at r -> 0 and
    returns 1 - |x| O(u) (measured: 1.6e-13 below 1 at x = 3072, exactly 1 at x = 1024 and 2048), and in fp32 Matern 3/2 and
    5/2 land one ulp below 1.  That is a property of the generating code at coordinates of 10^3 .. 10^7 length-scales, of no
    consequence at the coordinates of a real model; the designs of the Matern kernels avoid it with the `pow2` lattice, whose
    coordinates are powers of two: their product with 1 / sqrt 2 is exact, fused or not.
  * queries on unoccupied sites and at the origin see no source: exactly 1 + 2^-6, whatever the padded rows hold.

W[i, k] = wint[i, k] * mult[i] * 2^erow[i] (wint small integers, mult 1 or 2^p - 1), so that s2 = sum_i V^2 is a Python integer
times a power of two.  E is chosen per design as the largest exponent with s2 < 1/4 for every column: the clamp of the
variance at 0 cannot hide anything."""
from fractions import Fraction

import numpy as np

C, NOISE = 1.0, 2.0 ** -6
SPACING = 1024
ORIGIN = -1                          # query "site": the origin, 1024 or more away from every site
U64 = Fraction(1, 2 ** 53)           # unit roundoff of fp64


def gamma(k):
    return k * U64 / (1 - k * U64)


def lattice(n_sites, D, pow2=False):
    """integer coordinates of the sites 0 .. n_sites - 1: a line (D = 1), a square or a cubic grid, spacing 1024, first at 1024;
    pow2: every coordinate one of the 14 powers of two 2^10 .. 2^23 (gaps of 1024 and more), at most 14^D sites"""
    L = 1
    while L ** D < n_sites:
        L += 1
    assert not pow2 or L <= 14
    idx = np.arange(n_sites)
    xyz = np.stack([(idx // L ** d) % L for d in range(D)], axis=1)
    out = SPACING * (2 ** xyz if pow2 else 1 + xyz)
    assert out.max() < 2 ** 24
    return out.astype(np.float64)


class Design:
    """One model: sources on sites, an inverse factor, and the exact column sums of every site."""

    def __init__(self, name, N, D, site, wint, mult, eoff, n_empty=5, pow2=False):
        self.name, self.N, self.D = name + (" pow2" if pow2 else ""), N, D
        self._memo = {}
        self.site = np.asarray(site, dtype=np.int64)
        self.n_occupied = int(self.site.max()) + 1
        assert sorted(set(self.site.tolist())) == list(range(self.n_occupied))
        self.n_sites = self.n_occupied + n_empty
        self.coords = lattice(self.n_sites, D, pow2)
        self.X = self.coords[self.site]
        self.wint = wint                                    # (N, N) int8, lower triangular
        assert wint.shape == (N, N) and not np.triu(wint, 1).any()
        self.mult = [int(m) for m in mult]                  # Python integers, per row
        self.plain = all(m == 1 for m in self.mult)         # False: residue path only
        eoff = np.asarray(eoff, dtype=np.int64)
        # V in small integers: vs[i, g] = sum of wint[i, k] over the sources k of site g, and the sum of their magnitudes
        if self.n_occupied == N:
            self.vs = wint[:, np.argsort(self.site)]        # (int8: N = 8192 is 64 MiB)
            self.vabs_max = int(np.abs(wint).max())
        else:
            onehot = np.zeros((N, self.n_occupied), dtype=np.float32)
            onehot[np.arange(N), self.site] = 1.0
            self.vs = np.rint(wint.astype(np.float32) @ onehot).astype(np.int32)          # exact: integers up to N <= 2^24
            self.vabs_max = int(np.rint(np.abs(wint).astype(np.float32) @ onehot).max())
        # s2[g] = ints[g] 2^(2 (E + min eoff)): Python integers
        shift = 2 * (eoff - eoff.min())
        if self.plain and float(np.abs(self.vs).max()) ** 2 * 2.0 ** float(shift.max()) * N < 2.0 ** 62:
            ints = np.zeros(self.vs.shape[1], dtype=np.int64)
            for a in range(0, N, 512):                      # by row blocks: no (N, N) int64 temporary
                ints += ((self.vs[a:a + 512].astype(np.int64) ** 2) << shift[a:a + 512, None]).sum(axis=0)
            self.ints = [int(x) for x in ints]
        else:
            m2 = np.array([(m * m) << int(s) for m, s in zip(self.mult, shift)], dtype=object)
            self.ints = [int(x) for x in ((self.vs.astype(object) ** 2) * m2[:, None]).sum(axis=0)]
        # the largest E with max s2 < 1/4 (the unit of mult = 2^p - 1 rows is 2^-p of their exponent: eoff carries it)
        top = max(self.ints)
        self.E = -((top.bit_length() + 3) // 2) - int(eoff.min())
        self.erow = self.E + eoff
        self.unit_exp = 2 * int(self.erow.min())
        assert all(self.s2(g) < Fraction(1, 4) for g in range(self.n_occupied))

    def W(self):
        w = self.wint.astype(np.float64)
        w *= np.array([float(m) for m in self.mult])[:, None]        # 2^p - 1, p <= 50: exact
        return np.ldexp(w, self.erow[:, None].astype(np.int32))

    def s2(self, g):
        return Fraction(self.ints[g]) * Fraction(2) ** self.unit_exp if g >= 0 and g < self.n_occupied else Fraction(0)

    def queries(self, qsite):
        qsite = np.asarray(qsite, dtype=np.int64)
        Xq = self.coords[np.where(qsite < 0, 0, qsite)].copy()
        Xq[qsite < 0] = 0.0
        return Xq

    def kstar(self, qsite):
        """(N, M) kernel columns of these queries: ones and zeros"""
        return (self.site[:, None] == np.asarray(qsite)[None, :]).astype(np.float64)

    # ---- what a site's queries must return
    def check_exact(self, dtype):
        """The conditions under which k_var returns the reference bit for bit in `dtype`: every partial sum of V and of
        sum V^2, in any order, is an integer multiple of one unit below 2^53 (2^24), so no operation rounds."""
        assert self.plain, "rows of (1 - 2^-p) are for the residue path"
        lim = 2 ** 53 if dtype == np.float64 else 2 ** 24
        assert self.vabs_max < lim                                                     # V: units of 2^erow[i], per row
        assert max(self.ints) < lim                                                    # sum V^2: units of 2^unit_exp
        info = np.finfo(dtype)
        assert info.minexp < self.unit_exp and int(self.erow.min()) > info.minexp      # no underflow anywhere
        for g in range(self.n_occupied):
            v = Fraction(C) + Fraction(NOISE) - self.s2(g)
            assert Fraction(float(dtype(float(v)))) == v, f"{self.name}: the variance of site {g} is not a {dtype.__name__}"

    def expected(self, dtype):
        """fl(fl(c + noise) - s2) per site, as both finalizing kernels write it; index -1 (ORIGIN) and the empty sites: c + noise"""
        if dtype in self._memo:
            return self._memo[dtype]
        self.check_exact(dtype)
        a = dtype(C) + dtype(NOISE)
        out = np.empty(self.n_sites + 1, dtype=dtype)
        for g in range(self.n_sites):
            s2 = dtype(float(self.s2(g)))
            assert Fraction(float(s2)) == self.s2(g)
            out[g] = a - s2
        out[-1] = a
        self._memo[dtype] = out
        return out

    def check_i8(self, NP, p):
        """operands that are exactly p-bit integers after the path's scaling, and a product inside the moduli's range"""
        from tests import var_int8_restatement as r8
        assert p == r8.bits(NP) and NP >= self.N
        rowmax = np.array([float(m) for m in self.mult]) * np.abs(self.wint).max(axis=1)
        e = r8.exponent(np.ldexp(rowmax, self.erow.astype(np.int32)))
        wmax = np.abs(self.wint).max(axis=1)
        for i in range(self.N):
            # A'[i, k] = wint mult 2^(erow + p - e): an integer (sh >= 0) of at most 2^p
            sh = int(self.erow[i]) + p - int(e[i])
            assert sh >= 0 and (int(wmax[i]) * self.mult[i]) << sh <= 2 ** p
        assert NP * 4 ** p < r8.modulus_product() // 2

    def i8_reference(self, nbi):
        """Per site (index -1: the origin): the nearest double f of the exact variance, the remainder exact - f, and the bound
        (2 gamma_13 + gamma_d) s2 + u (c + noise) of test_var_exact.py's docstring, d = 16 + 2 + 8 + nbi."""
        if ("i8", nbi) in self._memo:
            return self._memo["i8", nbi]
        d = 16 + 2 + 8 + nbi
        f = np.empty(self.n_sites + 1)
        rem = np.empty(self.n_sites + 1)
        bound = np.empty(self.n_sites + 1)
        for g in list(range(self.n_sites)) + [-1]:
            s2 = self.s2(g)
            v = Fraction(C) + Fraction(NOISE) - s2
            f[g] = float(v)
            rem[g] = float(v - Fraction(float(v)))
            bound[g] = float((2 * gamma(13) + gamma(d)) * s2 + U64 * (Fraction(C) + Fraction(NOISE)))
        self._memo["i8", nbi] = (f, rem, bound)
        return f, rem, bound


def i8_error_over_bound(design, nbi, qsite, got):
    """max over the queries of |got - exact| / bound (<= 1 is the assertion), and where it is attained"""
    f, rem, bound = design.i8_reference(nbi)
    qsite = np.asarray(qsite)
    err = np.abs((np.asarray(got, dtype=np.float64) - f[qsite]) - rem[qsite])       # got - f is exact for neighbouring doubles
    ratio = err / bound[qsite]
    m = int(np.argmax(ratio))
    return float(ratio[m]), m


def f1(N, D=3, pow2=False):
    """one-hot: every source its own site; w random non-zero integers in [-8, 8], seed N"""
    rng = np.random.default_rng(N)
    w = rng.integers(1, 9, (N, N), dtype=np.int8)
    w *= rng.integers(0, 2, (N, N), dtype=np.int8) * np.int8(2) - np.int8(1)
    w = np.tril(w)
    return Design(f"F1 N={N} D={D}", N, D, np.arange(N), w, [1] * N, np.zeros(N, dtype=np.int64), pow2=pow2)


F2_OFFSETS = (0, 2, 5, 7)            # row exponents E_i - E (at most 12 apart)


def f2(N, G, interleaved=False, D=3, offsets=F2_OFFSETS, top_bits=0, pow2=False):
    """clusters: G sites, contiguous ranges or k mod G; saturated rows, all +, all - or alternating in k (row i: i mod 3), row
    exponents E + offsets[(i // 3) mod len].  top_bits = p > 0: every fifth row holds (1 - 2^-p) 2^(E_i) (residue path only)."""
    k = np.arange(N)
    site = k % G if interleaved else k * G // N
    sgn = np.ones((N, N), dtype=np.int8)
    sgn[1::3] = -1
    sgn[2::3, 1::2] = -1
    w = np.tril(sgn)
    eoff = np.array([offsets[(i // 3) % len(offsets)] for i in range(N)], dtype=np.int64)
    mult = [1] * N
    if top_bits:
        for i in range(4, N, 5):
            mult[i] = (1 << top_bits) - 1
            eoff[i] -= top_bits
    name = f"F2 N={N} G={G} {'interleaved' if interleaved else 'contiguous'} D={D}" + (f" top{top_bits}" if top_bits else "")
    return Design(name, N, D, site, w, mult, eoff, pow2=pow2)


def cycle_sites(design, M, stride=1):
    """M query sites cycling over all sites of the design, the empty ones and the origin included, in steps of `stride` - or of
    the next larger number that is coprime with the number of sites, so that the cycle visits every site (518 sites = 14 x 37
    would see 14 of them in steps of 37)"""
    import math
    total = design.n_sites + 1
    while math.gcd(stride, total) != 1:
        stride += 1
    out = (np.arange(M, dtype=np.int64) * stride) % total - 1
    assert len(np.unique(out)) == min(M, total)
    return out


def describe_wrong(design, qsite, got, want):
    """Failure message for the bit-for-bit tests: which columns are wrong, the sources they belong to, the tile (ib, kb), the row
    group and the k-step of those sources in the packed image of W, and the defect (got - want) / 2^unit as an integer: the
    sum of w^2 that went missing (positive) or was added (negative)."""
    got, want, qsite = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(qsite)
    bad = np.nonzero(~(got == want))[0]
    if bad.size == 0:
        return "all columns agree"
    lines = [f"{design.name}: {bad.size} of {got.size} columns wrong, first {bad[:8].tolist()}, last {int(bad[-1])}"]
    for m in bad[:6]:
        g = int(qsite[m])
        ks = np.nonzero(design.site == g)[0] if g >= 0 else np.array([], dtype=np.int64)
        where = "no source (empty site / origin)"
        if ks.size:
            k0, k1 = int(ks[0]), int(ks[-1])
            where = (f"{ks.size} source(s) k = {k0}..{k1}: tiles (ib >= {k0 // 512}, kb = {k0 // 512}..{k1 // 512}), row group "
                     f"{k0 % 512 // 64} of the diagonal tile, k-step {k0 % 512 // 4}" + (f"..{k1 % 512 // 4}" if k1 != k0 else ""))
        defect = (got[m] - want[m]) / 2.0 ** design.unit_exp
        lines.append(f"  column {int(m)} (site {g}): {where}; got {got[m]!r} want {want[m]!r}, defect {defect:.6g} units of 2^{design.unit_exp}")
    return "\n".join(lines)
