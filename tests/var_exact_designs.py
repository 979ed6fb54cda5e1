"""Operands for the variance kernels (k_var, k_var_i8) whose answer is known exactly, and that answer.  Host only: numpy and
Python integers / fractions.  Used by tests/test_var_exact_cpu.py (no GPU) and tests/test_var_exact.py (GPU), and - wide
lattices, per-task references, and everything under "derivative columns" at the end - by tests/test_var_exact_columns_cpu.py
and tests/test_var_exact_columns.py.

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


def lattice(n_sites, D, pow2=False, spacing=SPACING, star_at=1):
    """integer coordinates of the sites 0 .. n_sites - 1: a line (D = 1), a square or a cubic grid, spacing 1024, first at 1024;
    pow2: every coordinate one of the 14 powers of two 2^10 .. 2^23 (gaps of 1024 and more), at most 14^D sites.
    D >= 4 (the wide layouts): the digits of the site index alone leave most coordinates constant (1300 sites fill 11 binary
    digits of 15), and a coordinate that the generating sweep drops, or reads from another row of its query image, would
    change nothing.  So site 0 is the grid's corner and the D sites star_at .. star_at + D - 1 are its neighbours along each
    axis (the `star`); the other grid points follow in digit order.  separation() states what that buys."""
    if D >= 4:
        return _wide_lattice(n_sites, D, pow2, spacing, star_at)
    L = 1
    while L ** D < n_sites:
        L += 1
    assert not pow2 or L <= 14
    idx = np.arange(n_sites)
    xyz = np.stack([(idx // L ** d) % L for d in range(D)], axis=1)
    out = spacing * (2 ** xyz if pow2 else 1 + xyz)
    assert out.max() < 2 ** 24
    return out.astype(np.float64)


def _wide_lattice(n_sites, D, pow2, spacing, star_at):
    assert 1 <= star_at and star_at + D <= n_sites
    need = n_sites + D + 1
    L = 2
    while L ** D < need:
        L += 1
    assert not pow2 or L <= 14
    idx = np.arange(need)
    grid = np.stack([(idx // L ** d) % L for d in range(D)], axis=1)
    in_star = (grid.max(axis=1) <= 1) & (grid.sum(axis=1) <= 1)
    rest = grid[~in_star]
    xyz = np.concatenate([np.zeros((1, D), dtype=grid.dtype), rest[:star_at - 1], np.eye(D, dtype=grid.dtype), rest[star_at - 1:]])[:n_sites]
    assert len({tuple(r) for r in xyz.tolist()}) == n_sites
    out = spacing * (2 ** xyz if pow2 else 1 + xyz)
    assert out.max() < 2 ** 24
    return out.astype(np.float64)


def separation(coords, n_occupied):
    """Per coordinate d: (is there a pair of OCCUPIED sites that differ in d and agree in every other coordinate, is there such a
    pair of an occupied site and any site a query can sit on).  With the first, a source k and a query on another source's
    site are told apart by coordinate d alone: without d the query would see k at distance 0 and its column would gain
    W[., k].  A design with fewer than D + 1 occupied sites (all sources on one site, seven sites in D = 8) cannot have the
    first for every d - D directions need D + 1 points - and gets the second: its star sits on the empty sites, which the
    batches visit (an empty site that loses d returns an occupied site's variance, not c + noise)."""
    coords = np.asarray(coords)
    occ_occ, occ_any = [], []
    for d in range(coords.shape[1]):
        seen = {}
        for i, row in enumerate(np.delete(coords, d, axis=1).tolist()):
            seen.setdefault(tuple(row), []).append(i)
        groups = [g for g in seen.values() if len(g) > 1]
        occ_occ.append(any(sum(i < n_occupied for i in g) > 1 for g in groups))
        occ_any.append(any(min(g) < n_occupied for g in groups))
    return occ_occ, occ_any


class Design:
    """One model: sources on sites, an inverse factor, and the exact column sums of every site."""

    def __init__(self, name, N, D, site, wint, mult, eoff, n_empty=None, pow2=False, spacing=SPACING, e_shift=0):
        self.name, self.N, self.D = name + (" pow2" if pow2 else ""), N, D
        self._memo = {}
        self.site = np.asarray(site, dtype=np.int64)
        self.n_occupied = int(self.site.max()) + 1
        assert sorted(set(self.site.tolist())) == list(range(self.n_occupied))
        # wide layouts: the star of the lattice among the occupied sites where there are D + 1 of them, else on the first empty ones
        star_occupied = self.n_occupied >= D + 1
        if n_empty is None:
            n_empty = 5 if (D <= 3 or star_occupied) else max(5, D)
        self.n_sites = self.n_occupied + n_empty
        self.spacing = spacing
        self.coords = lattice(self.n_sites, D, pow2, spacing, 1 if star_occupied else self.n_occupied)
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
        # (e_shift: the derivative-column designs take s2 < 4^e_shift / 4, their columns are smaller than 1)
        self.E = -((top.bit_length() + 3) // 2) - int(eoff.min()) + e_shift
        self.erow = self.E + eoff
        self.unit_exp = 2 * int(self.erow.min())
        assert all(self.s2(g) < Fraction(4 ** e_shift, 4) for g in range(self.n_occupied))

    def W(self):
        w = self.wint.astype(np.float64)
        w *= np.array([float(m) for m in self.mult])[:, None]        # 2^p - 1, p <= 50: exact
        return np.ldexp(w, self.erow[:, None].astype(np.int32))

    def s2(self, g):
        return Fraction(self.ints[g]) * Fraction(2) ** self.unit_exp if g >= 0 and g < self.n_occupied else Fraction(0)

    def queries(self, qsite, delta=None):
        """the sites' coordinates (the origin for ORIGIN), moved by delta (M, D) where one is given"""
        qsite = np.asarray(qsite, dtype=np.int64)
        Xq = self.coords[np.where(qsite < 0, 0, qsite)].copy()
        Xq[qsite < 0] = 0.0
        return Xq if delta is None else Xq + delta

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


def f1(N, D=3, pow2=False, seed=None, unit=False, **kw):
    """one-hot: every source its own site; w random non-zero integers in [-8, 8] (unit: +-1), seed N unless one is given"""
    rng = np.random.default_rng(N if seed is None else seed)
    w = rng.integers(1, 9, (N, N), dtype=np.int8)
    if unit:
        w[:] = 1
    w *= rng.integers(0, 2, (N, N), dtype=np.int8) * np.int8(2) - np.int8(1)
    w = np.tril(w)
    name = f"{'U1' if unit else 'F1'} N={N} D={D}" + ("" if seed is None else f" seed {seed}")
    return Design(name, N, D, np.arange(N), w, [1] * N, np.zeros(N, dtype=np.int64), pow2=pow2, **kw)


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


# ---- multi-task models (gpt_fit_svgp): one design per task on shared sites ----------------------------------------------------------
def expected_task(design, c_t, noise, dtype):
    """What k_var_finalize writes for task t of a multi-task model whose factor slot holds c_t W (launch_pack_w's scale):
    s2 = c_t^2 sum V^2, var = fl(fl(c_t + noise) - s2), clamped at 0.  The conditions of check_exact, per task: c_t a power of two
    (the scaling of W and of every partial sum is exact), every partial sum of V and of sum V^2 a multiple of one unit below
    2^53 (2^24), nothing underflows after the scaling, s2 itself a number of the type.  Per site; the last entries (empty sites,
    ORIGIN): fl(c_t + noise)."""
    key = ("task", float(c_t), float(noise), dtype)
    if key in design._memo:
        return design._memo[key]
    assert design.plain
    m, e = np.frexp(float(c_t))
    assert m == 0.5, "outputscales are powers of two"
    lc = int(e) - 1
    lim = 2 ** 53 if dtype == np.float64 else 2 ** 24
    info = np.finfo(dtype)
    assert design.vabs_max < lim and max(design.ints) < lim
    assert info.minexp < design.unit_exp + 2 * lc and int(design.erow.min()) + lc > info.minexp
    a = dtype(c_t) + dtype(noise)
    out = np.empty(design.n_sites + 1, dtype=dtype)
    for g in range(design.n_sites):
        s2 = design.s2(g) * Fraction(c_t) ** 2
        assert Fraction(float(dtype(float(s2)))) == s2
        v = a - dtype(float(s2))
        assert v > 0
        out[g] = v
    out[-1] = a
    design._memo[key] = out
    return out


# ---- derivative columns: queries beside the sites ------------------------------------------------------------------------------------
# (tests/test_var_exact_columns.py has the derivation of everything below)
KT_RBF, KT_M32, KT_M52 = 0, 2, 3
G0 = {KT_RBF: 1.0, KT_M32: 3.0, KT_M52: 5.0 / 3.0}
SQRT_NU = {KT_M32: np.sqrt(np.longdouble(3)), KT_M52: np.sqrt(np.longdouble(5))}
EXP_REL_F64 = 3.5e-16                # gpt_exp.h: the table exp over [-745, 3]


def unit(dtype):
    return 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24


def gamma_f(k, u):
    return k * u / (1 - k * u)


def delta_magnitudes(D):
    """|delta_d|: distinct dyadic numbers.  D <= 3: 1/2, 1/4, 3/8; wide: (16 + d) / 128 = 0.125 .. 0.234 - small enough that g(|delta|)
    stays near g(0) in twelve dimensions, and neighbours differ by 1/17 or more: 60 times the fp32 operand bound."""
    return np.array([0.5, 0.25, 0.375][:D] if D <= 3 else [(16 + d) / 128 for d in range(D)])


def deltas(D, M):
    """(M, D) offsets: the magnitudes above with signs that change from query to query and from dimension to dimension"""
    m, d = np.arange(M)[:, None], np.arange(D)[None, :]
    sign = np.where((m * (d + 1) + m // 3 + d) % 2 == 0, 1.0, -1.0)
    return sign * delta_magnitudes(D)[None, :]


def column_reference(kt, delta):
    """longdouble k(|delta|) (M,) and the derivative columns g(|delta|) u_d, u = X - x = -delta (M, D); c = 1, l = 1"""
    dl = np.asarray(delta, dtype=np.longdouble)
    r2 = (dl * dl).sum(axis=1)
    if kt == KT_RBF:
        k = np.exp(-r2 / 2)
        g = k
    else:
        t = SQRT_NU[kt] * np.sqrt(r2)
        e = np.exp(-t)
        k = (1 + t) * e if kt == KT_M32 else (1 + t + t * t / 3) * e
        g = 3 * e if kt == KT_M32 else (np.longdouble(5) / 3) * (1 + t) * e
    return k, g[:, None] * -dl


def operand_bound(kt, dtype, delta, xmax):
    """Relative error bounds of the generated columns against column_reference, to first order: (k* column (M,), dk_d columns
    (M, D)).  xmax: the largest |coordinate| of a source or query."""
    u = unit(dtype)
    ad = np.abs(np.asarray(delta, dtype=np.float64))
    D = ad.shape[1]
    eps = 2 * u * xmax / ad                                  # d'_d = fl(x RS2) - fl(q RS2): two roundings of |x| RS2 against |delta_d| RS2
    h = (ad * ad).sum(axis=1) / 2
    dh = (ad * ad * eps).sum(axis=1) + (D + 2) * u * h      # 2 d' dd' per coordinate, and the products / fma of the sum
    if kt == KT_RBF:
        arg = h                                              # lnc = 0: the exponent is -h itself
        darg = dh
        pre_k = pre_g = 0.0
    else:
        t = float(SQRT_NU[kt]) * np.sqrt(2 * h)
        darg = t * (dh / (2 * h) + 4 * u)                    # sqrt (<= 1 ulp), the constant, the product
        arg = t
        if kt == KT_M32:
            pre_g = 0.0                                      # 3
            pre_k = darg / (1 + t) + u                       # 1 + t
        else:
            pre_g = darg / (1 + t) + 3 * u                   # (5/3) (1 + t)
            pre_k = darg * (1 + 2 * t / 3) / (1 + t + t * t / 3) + 5 * u
        pre_k, pre_g = pre_k + u, pre_g + u                  # prefactor times exponential
    # fp32: the argument times log2 e (the constant and the product: 2 u |arg|), then v_exp_f32 (1 ulp)
    e_exp = EXP_REL_F64 if dtype == np.float64 else 2 * u * arg + 2 * u
    rel_k = darg + e_exp + pre_k                             # the k* column is kv (1 + 0 . d'): nothing more
    rel_d = (darg + e_exp + pre_g)[:, None] + 3 * u + eps    # sqrt 2 / l (constant), its product with d'_d, kv times that
    return rel_k, rel_d


def underflow_distance(kt, dtype):
    """a source further than this from a query generates exactly 0 in every column: the exponent is below the point where the
    exp returns 0 (fp64: exp_tab, whose result is 0 below -745.2; fp32: v_exp_f32 returns 0 below 2^-149, taken at exponent
    -110 to be safe) and the prefactor is finite (matern_bound)"""
    need = 746.0 if dtype == np.float64 else 110.0
    return np.sqrt(2 * need) if kt == KT_RBF else need / float(SQRT_NU[kt])


def check_zero_off_site(design, kt, dtype, delta):
    """every source that is not on the query's site is further away than underflow_distance: sites differ by at least `spacing` in
    one coordinate, the query is at most max |delta_d| from its site in that coordinate"""
    gap = float(np.min(np.diff(np.unique(design.coords)))) if design.n_sites > 1 else design.spacing
    assert gap >= design.spacing
    nearest = design.spacing - float(np.abs(delta).max())
    assert nearest > underflow_distance(kt, dtype), (design.name, kt, dtype, nearest)
    # the queries' coordinates are numbers of the type, offsets included
    mag = np.abs(delta).max(axis=0)
    for sgn in (1.0, -1.0):
        Xq = design.coords + sgn * mag[None, :]
        assert np.array_equal(Xq.astype(dtype).astype(np.float64), Xq)


def calibration_exponents(prior, b2ref):
    """e with 4^e |b2| in (0.225, 0.9] prior: the calibrated s2 is within a factor 8 of the prior term and below it (var is clamped at 0)"""
    return np.floor(np.log2(0.9 * float(prior) / np.abs(np.asarray(b2ref, dtype=np.float64))) / 2).astype(np.int64)


class ColumnOutput:
    """One output array of one launch (var, Jvar or dvar of one task) against calibration: what must hold, elementwise.
    prior: the number the finalizing kernel subtracts from, in the model's type; b2ref: longdouble beta^2 (var, Jvar) or
    beta_0 beta_d (dvar) of column_reference; rel: the operand bound of that product; S (M, nblk): per query and i-block j above
    the source's own, sum over the block's rows i of (c_t W[i, k])^2, exact, as longdouble (0: no source, or no such block);
    subtract: out = prior - sum_j b2_j S_j (else out = -2 sum_j b2_j S_j).  b2_j: the operand as the rows of block j see it - a
    column block whose sweeps are shared out among workgroups is generated once per workgroup, by whichever of k_var's generating
    paths that workgroup's item takes, and the paths need not round alike (a product fused into a subtraction or not)."""

    def __init__(self, name, dtype, prior, b2ref, rel, S, subtract, c2=1.0):
        self.name, self.dtype, self.u, self.c2 = name, dtype, unit(dtype), float(c2)
        self.prior = np.longdouble(float(prior))
        self.b2ref, self.rel, self.subtract = b2ref, rel, subtract
        self.S = S
        self.nblk = S.shape[1]
        self.occ = np.broadcast_to(self.q(S.sum(axis=1) > 0), b2ref.shape)
        self.e = calibration_exponents((float(prior) if subtract else 1.0) / self.c2, b2ref)

    def q(self, v):
        """a per-query vector in the layout of this output: var (M,), Jvar (M, D), dvar (D, M)"""
        return v if self.b2ref.ndim == 1 else (v[None, :] if self.name == "dvar" else v[:, None])

    def calibrated(self, cal, j):
        """beta^2 as the rows of block j hold it, read back from the runs with W = 2^e (one row of block j per source) - the run of
        each element's own e - and the relative error of that reading: u for the one square, and u |output| / s2 for the final
        subtraction.  cal: {(e, j): output array}"""
        b2 = np.zeros(self.b2ref.shape, dtype=np.longdouble)
        crel = np.zeros(self.b2ref.shape)
        for e in np.unique(self.e):
            sel = self.e == e
            out = np.asarray(cal[int(e), j], dtype=np.longdouble)
            if self.subtract:
                s2 = self.prior - out
                with np.errstate(divide="ignore", invalid="ignore"):
                    cr = self.u + self.u * np.abs(out) / np.abs(s2)
                b = s2 / (np.longdouble(4.0) ** int(e) * np.longdouble(self.c2))
            else:
                b = out / (-2 * np.longdouble(4.0) ** int(e) * np.longdouble(self.c2))
                cr = np.full(out.shape, self.u)
            b2[sel], crel[sel] = b[sel], np.asarray(cr, dtype=np.float64)[sel]
        return b2, crel

    def check(self, cal, out, depth):
        """-> (worst operand error / bound, worst product error / bound); asserts the exact statements (no source: the prior)"""
        occ = self.occ
        out = np.asarray(out, dtype=np.longdouble)
        assert out.shape == self.b2ref.shape, (self.name, out.shape, self.b2ref.shape)
        empty_want = self.prior if self.subtract else np.longdouble(0)
        assert np.all(out[~occ] == empty_want), f"{self.name}: a query without a source does not return the prior"
        total = np.zeros(out.shape, dtype=np.longdouble)
        bound = self.u * np.abs(out).astype(np.float64) if self.subtract else np.zeros(out.shape)
        s2sum = np.zeros(out.shape)
        r_op = 0.0
        self.last_b2 = []
        for j in range(self.nblk):
            Sj = np.broadcast_to(self.q(self.S[:, j]), out.shape)
            has = Sj > 0
            b2, crel = self.calibrated(cal, j)
            assert np.all(b2[~occ] == 0), f"{self.name}: calibration of a query without a source"
            self.last_b2.append(b2)
            if not has.any():
                continue
            # operand: calibrated against the longdouble reference
            op_err = np.abs(b2 - self.b2ref)[has].astype(np.float64)
            op_bound = ((self.rel + crel) * np.abs(self.b2ref).astype(np.float64))[has]
            r_op = max(r_op, float(np.max(op_err / op_bound)))
            # product: (2 u_prod + gamma_(depth + 1) + 2 u_cal) s2, 2 u_cal = crel
            s2 = np.where(has, np.abs(b2 * Sj).astype(np.float64), 0.0)
            total += np.where(has, b2 * Sj, 0)
            bound = bound + (2 * self.u + gamma_f(depth + 1, self.u) + np.where(has, crel, 0.0)) * s2
            s2sum += s2
        est = self.prior - total if self.subtract else -2 * total
        err = np.abs(out - est).astype(np.float64)
        self.last = dict(bound=bound, s2=s2sum)
        r_pr = float(np.max(err[occ] / bound[occ])) if occ.any() else 0.0
        return r_op, r_pr

    def discrimination(self, min_w2, bound):
        """smallest change of an output that one dropped or doubled (i, k) term makes, over 16 bounds: min over the rows of
        (W[i, k])^2 (c^2 included) times |b2| (a dropped term takes V_i^2 away, a doubled one adds 3 V_i^2; dvar: twice that),
        elementwise minimum of the ratio over the queries with a source"""
        change = np.abs(self.b2ref).astype(np.float64) * np.broadcast_to(self.q(min_w2), self.b2ref.shape) * (1.0 if self.subtract else 2.0)
        occ = self.occ
        return float(np.min(change[occ] / (16 * bound[occ]))) if occ.any() else np.inf


def site_sums(design, qsite, c_t=1.0):
    """per query: S (M, nbi) - for the source k of the query's site and j = 0 .. nbi - 1, the sum of (c_t W[i, k])^2 over the rows of
    i-block k // 512 + j, as longdouble (exact: integers below 2^63 times a power of two; 0 where there is no source or no such
    block) - and the smallest (c_t W[i, k])^2 of that source: one-hot designs, whose every term is a V_i of its own"""
    assert design.n_occupied == design.N and np.array_equal(design.site, np.arange(design.N)), "one source per site, source k on site k"
    assert np.all(design.erow == design.E)
    key = ("site_sums", float(c_t))
    if key not in design._memo:
        N = design.N
        nbi = -(-N // 512)
        w2 = design.wint.astype(np.int64) ** 2
        blk = np.stack([w2[512 * b:512 * (b + 1)].sum(axis=0) for b in range(nbi)], axis=1)          # (k, block)
        assert np.array_equal(blk.sum(axis=1), np.array(design.ints, dtype=np.int64))
        n_all = design.n_sites + 1
        S = np.zeros((n_all, nbi), dtype=np.longdouble)
        kb = np.arange(N) // 512
        for j in range(nbi):
            ok = kb + j < nbi
            S[:N, j][ok] = blk[np.arange(N)[ok], (kb + j)[ok]]
        S *= np.longdouble(4.0) ** design.E * np.longdouble(float(c_t)) ** 2
        a = np.abs(design.wint).astype(np.int16)
        a[a == 0] = 127
        minw = np.r_[a.min(axis=0).astype(np.float64) ** 2 * 4.0 ** design.E * float(c_t) ** 2, np.zeros(n_all - N)]
        design._memo[key] = (S, minw)
    S, minw = design._memo[key]
    qsite = np.asarray(qsite)
    return S[qsite], minw[qsite]


def calibration_rows(N, j):
    """(rows, sources): for every source k whose i-block k // 512 + j exists, the first row of that block at or below the diagonal"""
    k = np.arange(N)
    ib = k // 512 + j
    ok = 512 * ib < N
    return np.maximum(k, 512 * ib)[ok], k[ok]


def calibration_factor(N, e, j):
    """the factor of a calibration run: 2^e at one row of block k // 512 + j in every column k (j = 0: 2^e I)"""
    W = np.zeros((N, N))
    rows, cols = calibration_rows(N, j)
    W[rows, cols] = 2.0 ** e
    return W


def column_outputs(design, kt, dtype, qsite, delta, flags, c_t=1.0, noise=NOISE):
    """the ColumnOutput of every variance output a request returns, for one task (outputscale c_t: the columns are generated
    with c = 1 and the factor carries c_t, as gpt_fit_svgp packs it; a single-task model has c_t = c = 1)"""
    k, dk = column_reference(kt, delta)
    xmax = float(np.abs(design.queries(qsite, delta)).max())
    rel_k, rel_d = operand_bound(kt, dtype, delta, max(xmax, float(design.coords.max())))
    S, _ = site_sums(design, qsite, c_t)
    res = {}
    if flags.get("var"):
        res["var"] = ColumnOutput("var", dtype, dtype(c_t) + dtype(noise), k * k, 2 * rel_k, S, True, c_t ** 2)
    if flags.get("Jvar"):
        res["Jvar"] = ColumnOutput("Jvar", dtype, dtype(c_t) * dtype(G0[kt]), dk * dk, 2 * rel_d, S, True, c_t ** 2)
    if flags.get("dvar"):
        res["dvar"] = ColumnOutput("dvar", dtype, 0.0, (k[:, None] * dk).T, (rel_k[:, None] + rel_d).T, S, False, c_t ** 2)
    return res


def chain_depth(plan, nbi):
    """the longest chain of additions from a square to an output (test_var_exact_columns.py): 16 squares per lane and sweep, nbi
    sweeps, two shuffle additions, eight waves, the slots k_var_finalize adds (one for a block of a whole round)"""
    fin = plan["fin"]
    slots = int((fin[:, 1] - fin[:, 0]).max()) if len(fin) else 1
    return 16 * nbi + 2 + 8 + max(slots, 1)


def restate_columns(design, kt, dtype, qsite, delta, flags, W, c_t=1.0, noise=NOISE):
    """numpy restatement of one launch in the model's type: the columns generated as k_var does (scaled coordinates, their
    difference, one exp), V = (c_t W) B one product per row (one-hot), squares and cross products summed pairwise,
    k_var_finalize's last line.  W: a dense factor, or (e, j) for calibration_factor(N, e, j)."""
    T = dtype
    rs2 = T(0.70710678118654752440)
    X = design.coords[np.where(np.asarray(qsite) < 0, 0, qsite)].astype(T)
    Xq = design.queries(qsite, delta).astype(T)
    dd = X * rs2 - Xq * rs2                                   # (M, D) the source on the query's site
    h = (dd * dd).sum(axis=1, dtype=T)
    if kt == KT_RBF:
        kv = np.exp(-h).astype(T)
        gv = kv
    else:
        t = (T(float(SQRT_NU[kt])) * np.sqrt(h + h)).astype(T)
        e = np.exp(-t).astype(T)
        kv = ((T(1) + t) * e if kt == KT_M32 else (T(1) + t + t * t * T(1.0 / 3.0)) * e).astype(T)
        gv = (T(3) * e if kt == KT_M32 else T(5.0 / 3.0) * (T(1) + t) * e).astype(T)
    cols = np.concatenate([kv[:, None], gv[:, None] * (T(1.41421356237309504880) * dd)], axis=1).astype(T)      # (M, 1 + D)
    qs = np.asarray(qsite)
    occ = np.nonzero((qs >= 0) & (qs < design.n_occupied))[0]
    out = {}
    M, D = dd.shape
    s2 = np.zeros((M, 1 + D), dtype=T)
    cr = np.zeros((M, D), dtype=T)
    if isinstance(W, tuple):
        e, j = W
        occ = occ[512 * (qs[occ] // 512 + j) < design.N]                            # the sources whose block j exists
        V = (T(2.0 ** int(e)) * T(c_t)) * cols[occ]                                # the one row with a source: adding zeros changes nothing
        s2[occ] = V * V
        cr[occ] = V[:, :1] * V[:, 1:]
    else:
        Wt = (W * c_t).astype(T)
        for a in range(0, occ.size, 64):
            m = occ[a:a + 64]
            # along contiguous rows numpy adds pairwise (eight interleaved chains of 16 per block of 128, then a tree): shorter than
            # the kernel's chain.  Down the columns of a C-ordered array it would add row after row, a chain of N.
            Vt = np.ascontiguousarray((Wt[:, qs[m]][:, :, None] * cols[m][None, :, :]).transpose(1, 2, 0))      # (queries, 1 + D, N)
            s2[m] = (Vt * Vt).sum(axis=2, dtype=T)
            cr[m] = (Vt[:, :1] * Vt[:, 1:]).sum(axis=2, dtype=T)
    if flags.get("var"):
        out["var"] = np.maximum((T(c_t) + T(noise)) - s2[:, 0], T(0))
    if flags.get("Jvar"):
        out["Jvar"] = T(c_t) * T(G0[kt]) - s2[:, 1:]
    if flags.get("dvar"):
        out["dvar"] = (T(-2) * cr).T
    return out


# ---- launch kinds and batch sizes of the derivative-column tests -----------------------------------------------------------------
# the requests of tests/test_kernel_dispatch.py that reach k_var with derivative columns
REQUESTS = (dict(Jvar=True), dict(J=True, Jvar=True), dict(var=True, Jvar=True), dict(J=True, Jvar=True, dvar=True))
TAIL_CUT_COLUMNS = (460, 300, 700, 1000)
ROUNDS_COLUMNS = (16500, 17000, 20000, 33000, 50000, 40000, 70000)


def request_name(flags):
    return " + ".join(k for k in ("mean", "var", "J", "Jvar", "dvar") if flags.get(k))


def cols_per_query(D, flags):
    """columns of k_var per query (gpt_predict_all's choice): the fused layout (k*, dk_0 .. and zero columns up to 4 / 8 / 16) when var
    or dvar is asked for, else the derivative columns alone (D for D <= 3, 4 and 8 for D = 4 and 8, the fused layout otherwise);
    1 for var alone"""
    if not (flags.get("Jvar") or flags.get("dvar")):
        return 1
    fused = 4 if D <= 3 else (8 if D <= 7 else 16)
    alone = D if D <= 3 else (4 if D == 4 else (8 if D == 8 else fused))
    return fused if (flags.get("var") or flags.get("dvar")) else alone


def plan_features(plan):
    return {"tail_cut": plan["nfull"] == 0 and plan["n_splits"] > 0 and plan["cut_diag"],
            "rounds_and_tail": 0 < plan["nfull"] < plan["ncb"]}


def pick_queries(feature, cpq, nbi, ntask, P):
    """the first candidate number of queries whose plan (for its cpq M columns) has the feature, and that plan; None if none has"""
    from gaussian_process_transportation_amd import _lib
    for cols in (TAIL_CUT_COLUMNS if feature == "tail_cut" else ROUNDS_COLUMNS):
        M = -(-cols // cpq)
        plan = _lib.debug_var_plan(M * cpq, nbi, ntask, P)
        if plan_features(plan)[feature]:
            return M, plan
    return None


def column_batches(D, flags, nbi, ntask, P, n_sites_all):
    """query counts of one launch kind: 1, the count that fills one 64-column block and one more, one query per site (n_sites_all:
    every (i, k) term of the factor is in some column), one with a tail cut along k and one with whole rounds and a tail - and the
    longest chain of additions over their plans"""
    from gaussian_process_transportation_amd import _lib
    cpq = cols_per_query(D, flags)
    Ms = [1, 64 // cpq, 64 // cpq + 1, n_sites_all]
    depth = max(chain_depth(_lib.debug_var_plan(M * cpq, nbi, ntask, P), nbi) for M in Ms)
    for feature in ("tail_cut", "rounds_and_tail"):
        got = pick_queries(feature, cpq, nbi, ntask, P)
        assert got is not None, f"no candidate batch has the plan feature {feature} at {cpq} columns per query, nbi = {nbi}, {ntask} task(s), {P} workgroups"
        Ms.append(got[0])
        depth = max(depth, chain_depth(got[1], nbi))
    return Ms, depth


def column_sites(design, M):
    """M query sites: a cycle over all sites (empty ones and the origin included) that starts at another place for every M"""
    total = design.n_sites + 1
    return np.roll(cycle_sites(design, total, 37), 11 * M)[:M] if M <= total else cycle_sites(design, M, 37)


def column_design(N, D, dtype, seed=None, c_t=1.0):
    """the design of the derivative-column tests: one-hot, s2 < 1; fp64: F1 on the 1024-lattice; fp32: |w| = 1 (F1's w in [-8, 8] fails
    the discrimination condition there) on a 128-lattice, which keeps the coordinate term of the operand bound small.  A task with
    outputscale c_t < 1 takes s2 < 1 / c_t: its outputs are c_t (prior) - c_t^2 s2, and with s2 < 1 the subtracted part would be
    c_t times smaller against the rounding of the prior than in a single-task model (fp32, c_t = 1 / 4: below 16 bounds)."""
    f32 = dtype == np.float32
    return f1(N, D, seed=seed, unit=f32, spacing=128 if f32 else SPACING, e_shift=1 + max(0, int(round(-np.log2(c_t) / 2))))


def pow2_sites(design):
    """the occupied sites whose coordinates are all powers of two: their scaled coordinates are exact, a query on them sees a
    distance of exactly 0 however the generating code rounds or fuses"""
    m, _ = np.frexp(design.coords[:design.n_occupied])
    return np.nonzero(np.all(m == 0.5, axis=1))[0]
