"""Input sets of the fold-scan tests, their longdouble reference and the tolerances derived from it.  Shared, read-only, by
tests/test_fold_scan_cpu.py (which asserts the conditions stated here, without a GPU) and tests/test_fold_scan.py (the kernels).

Inputs follow tests/test_batch_precision.py: sources in [0, 1]^D, ls_d in U(0.3, 0.6) sqrt(D), c in U(0.05, 0.2), noise in
U(5e-4, 5e-3), so that cond(K) <= c n / noise < 5e4 and an fp64 evaluation stays within 1e-11 of the longdouble one; queries in
U(-0.1, 1.1)^D.  The displacement is 0.3 sin(4 x + phase) + 0.03 N(0, 1): its slope reaches 1.2, so the map folds at some queries
and not at others and n_fold is neither 0 nor M_b (asserted for the members that have enough queries to tell).

Tolerances, test_batch_precision.py's rule: a quantity q of member b is held to

    tol(q, b) = 32 * max(e_oracle(q, b), n_b * 2^-53)                (never above 1e-9)

relative to the largest magnitude of the reference array, where e_oracle is the distance of the same computation in plain fp64
(fold_scan_restatement.scan_fp64) from the longdouble restatement, which tests/test_fold_scan_cpu.py holds to 40-digit mpmath.
(The longdouble restatement's own distance from mpmath is 1e-17 or less, far under n 2^-53; taken literally as e_oracle it would
reduce the rule to 32 n 2^-53 = 1e-13 at n = 33, below cond(K) 2^-53 = 5e-12, which no fp64 factorisation can meet.  As in
test_batch_precision.py, e_oracle measures what fp64 resolves on the case.)  The kernel does not return J; det = det(I + J) is
held to J's bound pushed through first order, per query:

    |det - det_ref| <= D * max(1, |I + J|_F)^(D - 1) * tol(J, b) * max |J|

(each of the D! products of det has D factors bounded by |I + J|_F; perturbing one factor by dJ changes det by at most
D |I + J|_F^(D - 1) |dJ| to first order).  err_sum is a sum of M_b values each within tol(err) max err of its reference, added in
fp64: M_b (tol(err) max err + 2^-53 err_sum)."""
import functools
import zlib

import numpy as np

from tests import fold_scan_restatement as fr

LD = fr.LD
JITTER = 1e-10
FACTOR, CAP, ORACLE_BOUND = 32.0, 1e-9, 1e-11
QT = 64                                                    # queries of one fs_scan tile (csrc/gpt_batch.h BAT_QT)
SIZES = (1, 2, 31, 32, 33, 127, 128)                       # both size classes and their edges
QUERIES = (0, 1, QT - 1, QT, QT + 1, 3 * QT + 1, QT)       # M_b: none, one, a tile less one, a tile, one more, three tiles and one
WIDTHS = ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3))          # (D, n_ls)


def draw_model(rng, n, D, n_ls):
    X = rng.uniform(0, 1, (n, D))
    Y = 0.3 * np.sin(4 * X + np.arange(D)) + 0.03 * rng.standard_normal((n, D))
    return X, Y, rng.uniform(0.3, 0.6, n_ls) * np.sqrt(D), rng.uniform(0.05, 0.2), rng.uniform(5e-4, 5e-3)


def draw_batch(key, sizes, D, n_ls, queries):
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    Xs, Ys, ls, c, noise = map(list, zip(*(draw_model(rng, n, D, n_ls) for n in sizes)))
    xqs = [rng.uniform(-0.1, 1.1, (m, D)) for m in queries]
    return dict(Xs=Xs, Ys=Ys, ls=np.array(ls), c=np.array(c), noise=np.array(noise), xqs=xqs, D=D)


SPECS = {f"sizes-D{D}-{'iso' if n_ls == 1 else 'ard'}": functools.partial(draw_batch, f"sizes-{D}-{n_ls}", SIZES, D, n_ls, QUERIES)
         for D, n_ls in WIDTHS}
SPECS["shared-B2"] = functools.partial(draw_batch, "shared-2", (20, 33), 2, 2, (3 * QT + 1,))      # one query set for both members
SPECS["shared-B1"] = functools.partial(draw_batch, "shared-1", (20,), 3, 3, (QT + 1,))
CASES = sorted(SPECS)


def queries_of(s, b):
    return s["xqs"][b if len(s["xqs"]) == len(s["Xs"]) else 0]


def tolerance(e_oracle, n):
    return FACTOR * max(e_oracle, n * 2.0 ** -53)


def relerr(got, want):
    want = np.asarray(want, dtype=LD)
    if want.size == 0:
        return 0.0
    den = np.max(np.abs(want))
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - want)) / (den if den > 0 else LD(1)))


@functools.lru_cache(maxsize=None)
def case(cid):
    """The inputs of a case, the longdouble reference per member and the fp64 evaluation's error against it per quantity.
    Computed once per process."""
    s = SPECS[cid]()
    s["ref"], s["e_oracle"] = [], []
    for b in range(len(s["Xs"])):
        args = (s["Xs"][b], s["Ys"][b], s["c"][b], s["ls"][b], s["noise"][b], JITTER, queries_of(s, b))
        ref, o = fr.scan(*args), fr.scan_fp64(*args)
        assert ref["status"] == fr.OK and ref["surrogate_status"] == fr.OK
        s["ref"].append(ref)
        s["e_oracle"].append({q: relerr(o[q], ref[q]) for q in ("J", "z", "err", "psi")})
    return s


def det_bound(ref, tol_J):
    """Per query: D max(1, |I + J|_F)^(D - 1) tol(J) max |J|."""
    J = ref["J"]
    if J.shape[0] == 0:
        return np.zeros(0)
    D = J.shape[-1]
    F = np.sqrt(((J + np.eye(D, dtype=LD)) ** 2).sum((-1, -2))).astype(np.float64)
    return D * np.maximum(1.0, F) ** (D - 1) * tol_J * float(np.max(np.abs(J)))
