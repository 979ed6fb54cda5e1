"""numpy restatement of the residue (int8) variance product (csrc/gpt_plan_i8.h, gpt_kvar_i8.h).

V = W K*^T is taken exactly in integers: rows of W and kernel columns are rounded to p-bit integers A', B' against a
power-of-two bound each, the integer product is formed modulo 14 pairwise coprime moduli that fit int8 (one int8 GEMM with
int32 sums per modulus), rebuilt by Garner's mixed-radix conversion in balanced digits and scaled back.

Column exponent: ONE value f from the prior variance, 2^f >= c >= k* (COLUMN_EXPONENT).  The column's own maximum keeps the
relative accuracy of columns far from the data, which the variance does not need: var = c + noise - |V|^2 is wanted to an
absolute bound, and test_var_int8_cpu.py measures both choices (N = 1024, M = 64, worst |var - 80-bit product|: 1.5e-15
with the prior variance, 1.3e-15 with the column's maximum, 3.7e-16 for the fp64 product: 600 times inside the 1e-12 bound).  The prior variance needs no pass over the column before it is quantised, so the kernel uses it."""
import numpy as np

MODULI = (256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199)
MIN_BITS = 44
MAX_NP = 16384                      # the largest padded model the path takes (32 i-blocks of 512 rows)
COLUMN_EXPONENT = "prior"           # or "column"


def modulus_product():
    m = 1
    for x in MODULI:
        m *= x
    return m


def bits(NP):
    """p = floor((log2 M - 1 - ceil(log2 NP)) / 2): NP 2^(2p) < M / 2."""
    lg = int(np.ceil(np.log2(NP)))
    return int(np.floor((np.log2(float(modulus_product())) - 1 - lg) / 2))


def exponent(x):
    """smallest integer e with x <= 2^e (0 for x == 0)"""
    x = np.asarray(x, dtype=np.float64)
    f, e = np.frexp(x)
    e = np.where(f == 0.5, e - 1, e)
    return np.where(x > 0, e, 0).astype(np.int64)


def quantise_rows(W, p):
    e = exponent(np.max(np.abs(W), axis=1))
    A = np.rint(np.ldexp(W, (p - e)[:, None])).astype(np.int64)
    return A, e


def quantise_columns(Kst, p, c, how=COLUMN_EXPONENT):
    """Kst: (N, M) kernel columns.  Returns B' (N, M) and f (M,)"""
    if how == "prior":
        f = np.full(Kst.shape[1], int(exponent(c)), dtype=np.int64)
    else:
        f = exponent(np.max(np.abs(Kst), axis=0))
    B = np.rint(np.ldexp(Kst, (p - f)[None, :])).astype(np.int64)
    return B, f


def balanced(x, m):
    """residue of the integers x modulo m in [-(m // 2), (m - 1) // 2] (fits int8 for every modulus)"""
    r = np.mod(x, m)
    return np.where(r > (m - 1) // 2, r - m, r)


def planes(X):
    return [balanced(X, m).astype(np.int8) for m in MODULI]


def plane_sums(Ap, Bp):
    """C_j = A_j B_j in int32, as the int8 matrix instruction accumulates it (the bound 128^2 K < 2^31 is asserted);
    taken in fp64, which is exact below 2^53"""
    out = []
    for a, b in zip(Ap, Bp):
        c = a.astype(np.float64) @ b.astype(np.float64)
        assert np.max(np.abs(c)) < 2.0 ** 31
        out.append(c.astype(np.int64).astype(np.int32))
    return out


def garner_digits(res):
    """res[j]: integer arrays, residues modulo MODULI[j].  Balanced mixed-radix digits d_j:
    C = d_0 + m_0 (d_1 + m_1 (d_2 + ...))."""
    d = []
    for i, m in enumerate(MODULI):
        s = np.zeros_like(res[0], dtype=np.int64)
        prod = 1
        for l in range(i):
            s = s + d[l] * int(balanced(np.int64(prod), m))
            prod = prod * MODULI[l] % m
        inv = pow(prod, -1, m) if i else 1
        d.append(balanced((res[i].astype(np.int64) - s) * int(balanced(np.int64(inv), m)), m))
    return d


def horner_exact(d):
    """the integer the digits stand for, as Python integers (object array)"""
    x = d[-1].astype(object)
    for i in range(len(MODULI) - 2, -1, -1):
        x = x * MODULI[i] + d[i].astype(object)
    return x


def horner_fp64(d):
    x = d[-1].astype(np.float64)
    for i in range(len(MODULI) - 2, -1, -1):
        x = x * float(MODULI[i]) + d[i].astype(np.float64)
    return x


def integer_product(A, B, exact=False):
    """sum_k A'[i, k] B'[k, m] rebuilt from the 14 int32 plane sums: fp64 (Horner) or exact Python integers"""
    C = plane_sums(planes(A), planes(B))
    d = garner_digits([balanced(c.astype(np.int64), m) for c, m in zip(C, MODULI)])
    return horner_exact(d) if exact else horner_fp64(d)


def product(W, Kst, c, NP, how=COLUMN_EXPONENT):
    """V = W K*^T (N, M) by the residue scheme"""
    p = bits(NP)
    assert p >= MIN_BITS
    A, e = quantise_rows(W, p)
    B, f = quantise_columns(Kst, p, c, how)
    return np.ldexp(integer_product(A, B), e[:, None] + f[None, :] - 2 * p)


def variance(W, Kst, c, noise, NP, how=COLUMN_EXPONENT):
    V = product(W, Kst, c, NP, how)
    v = c + noise - np.sum(V * V, axis=0)
    return np.where(v < 0, 0.0, v)


def variance_quantised(W, Kst, c, noise, NP, how=COLUMN_EXPONENT):
    """The same quantised operands, their product taken by an fp64 GEMM instead of the residues: what large batches are checked
    against (the residue pipeline costs 14 products and a reconstruction).  Differs from variance() by the rounding of one
    fp64 dot product per element, 1e-16 relative; test_var_int8_cpu.py holds the two together."""
    p = bits(NP)
    A, e = quantise_rows(W, p)
    B, f = quantise_columns(Kst, p, c, how)
    V = np.ldexp(A.astype(np.float64), (e - p)[:, None]) @ np.ldexp(B.astype(np.float64), (f - p)[None, :])
    v = c + noise - np.sum(V * V, axis=0)
    return np.where(v < 0, 0.0, v)
