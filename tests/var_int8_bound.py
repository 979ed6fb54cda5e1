"""Derived error bounds for the residue (int8) variance path on real models (host only, numpy), and the models of
tests/test_var_int8_gpu.py::test_other_shapes_kernels_and_scales / tests/test_var_int8_cpu.py that use them.

1. Quantisation (restatement against a long-double product).  A' = W 2^(p - e_i) + a, B' = k 2^(p - f) + b with |a|, |b| <= 1/2,
   so A' B' 2^(e_i + f - 2p) - W k = a k 2^(e_i - p) + b W 2^(f - p) + a b 2^(e_i + f - 2p), and per element of V
       |dV_i| <= 2^(-p-1) (2^f sum_k |W_ik| + 2^(e_i) sum_k |k_k|)  +  N 2^(e_i + f - 2p - 2);
   the restatement adds Horner's 13 roundings (two each without fma: gamma_26 |V_i|).

2. Device against restatement, given the SAME W (the handle's export) and the oracle's k*.  A' is the same integer matrix on
   both sides and the integer product is exact, so they differ by three things:
   a. The kernel value.  Both sides evaluate c k(|z_x - z_q|), z = x / l, in fp64, by different routes.  With
      G = sum_d |dz_d| (|z_x,d| + |z_q,d|) and r^2 = sum_d dz_d^2:
        device (gpt_kvar_i8.h): xs = fl(x fl(1/l)), q = fl(xq fl(fl(1/l) / sqrt 2)), d = xs / sqrt 2 - q (fused or not), h = sum d^2 by
        fma: |dh| <= u (4 G + 2.5 r^2);  oracle: z = fl(x / l), cdist: |d(r^2 / 2)| <= u (G + 3 r^2).
      RBF: the argument of exp is lnc - h; fl(log c) and the subtraction add u (2 |lnc| + r^2 / 2); exp_tab is 3.5e-16 = 3.2 u
      relative, numpy's exp and its product with c 3 u:   eps = u (5 G + 6 r^2 + 2 |lnc| + 7).
      Matern: r = sqrt(r^2) has |dr| <= d(r^2) / (2 r) + u r on each side, t = kappa r adds 2 u t, and t enters the exponent and
      the polynomial P (P' / P <= 1):   eps = 2 (dt_dev + dt_orc) + u (2 |lnc| + t + 18),  dt = kappa d(r^2) / (2 r) + 3 u t.
   b. One unit of B' wherever the two values land across a rounding boundary: with x = k 2^(p - f) and delta = eps x,
      |B'_dev - B'| <= delta + [a half-integer lies within delta of x].
   c. Horner with fma (device, 13 roundings) against multiply-add (restatement, 26): 39 u |V_i|, taken as 40 u.
   So |dV_i| <= 2^(e_i + f - 2p) sum_k |A'_ik| (delta_k + cross_k) + 40 u |V_i|, and
       |var_dev - var| <= sum_i (2 |V_i| |dV_i| + dV_i^2) + (gamma_(N+1) + gamma_d) s2 + 2 u (c + noise):
   the restatement adds its N squares row by row, the device in its tree of depth d = 16 + 2 + 8 + nbi (test_var_exact.py), and
   each side subtracts once.  The clamp at 0 is 1-Lipschitz."""
import numpy as np

from oracle import gp_oracle as orc
from tests import var_int8_restatement as r8

U = 2.0 ** -53
KAPPA = {"matern12": 1.0, "matern32": np.sqrt(3.0), "matern52": np.sqrt(5.0)}
KINDS = ("rbf", "matern12", "matern32", "matern52")

# name, N, D, kernel, length-scale, c  (noise = 1e-3 c, jitter 1e-10 c)
CASES = [("D1", 512, 1, "rbf", (0.1,), 0.1), ("D2", 512, 2, "rbf", (0.1, 0.1), 0.1),
         ("matern12", 512, 3, "matern12", (0.1, 0.1, 0.1), 0.1), ("matern32", 512, 3, "matern32", (0.1, 0.1, 0.1), 0.1),
         ("aniso", 1024, 3, "rbf", (0.05, 0.2, 0.8), 0.1), ("c_small", 512, 3, "rbf", (0.1, 0.1, 0.1), 2.0 ** -20 * 1.3),
         ("c_four", 512, 3, "rbf", (0.1, 0.1, 0.1), 4.0), ("c_large", 1024, 3, "rbf", (0.1, 0.1, 0.1), 3e5)]
BATCHES = (1, 129, 300)


def case_problem(case):
    name, N, D, kind, ls, c = case
    X, Y, Xq = orc.synthetic_problem(N, max(BATCHES), D=D)
    return dict(name=name, N=N, NP=-(-N // 512) * 512, D=D, kind=kind, ls=np.array(ls), c=c, noise=1e-3 * c, jitter=1e-10 * c, X=X, Y=Y, Xq=Xq)


def gamma(k):
    return k * U / (1 - k * U)


def quantisation_bound(W, Kst, c, NP):
    """(N, M): the bound of 1. on |V_restatement - V| per element"""
    p = r8.bits(NP)
    e = r8.exponent(np.max(np.abs(W), axis=1)).astype(np.float64)
    f = float(r8.exponent(c))
    N = W.shape[0]
    rows = np.sum(np.abs(W), axis=1)[:, None]
    cols = np.sum(np.abs(Kst), axis=0)[None, :]
    first = 2.0 ** (-p - 1) * (2.0 ** f * rows + 2.0 ** e[:, None] * cols)
    return first + N * 2.0 ** (e[:, None] + f - 2 * p - 2)


def kernel_rel_error(X, Xq, ls, c, kind):
    """(N, M): eps of 2a."""
    z, zq = X / ls, Xq / ls
    G = np.zeros((X.shape[0], Xq.shape[0]))
    r2 = np.zeros_like(G)
    for d in range(X.shape[1]):
        dz = np.abs(z[:, None, d] - zq[None, :, d])
        G += dz * (np.abs(z[:, None, d]) + np.abs(zq[None, :, d]))
        r2 += dz * dz
    lnc = abs(np.log(c))
    if kind == "rbf":
        return U * (5 * G + 6 * r2 + 2 * lnc + 7)
    r = np.sqrt(r2)
    t = KAPPA[kind] * r
    safe = np.where(r > 0, r, 1.0)
    dt_dev = KAPPA[kind] * np.where(r > 0, U * (8 * G + 5 * r2) / (2 * safe), np.sqrt(U * (8 * G + 5 * r2))) + 3 * U * t
    dt_orc = KAPPA[kind] * np.where(r > 0, U * (2 * G + 6 * r2) / (2 * safe), np.sqrt(U * (2 * G + 6 * r2))) + 3 * U * t
    return 2 * (dt_dev + dt_orc) + U * (2 * lnc + t + 18)


def device_bound(W, Kst, eps, c, noise, NP):
    """(M,): the bound of 2. on |var_device - var_restatement|"""
    p = r8.bits(NP)
    N = W.shape[0]
    A, e = r8.quantise_rows(W, p)
    f = int(r8.exponent(c))
    x = np.ldexp(Kst, p - f)
    delta = eps * x
    cross = np.abs(x - np.floor(x) - 0.5) <= delta
    dB = delta + cross
    V = r8.product(W, Kst, c, NP)
    dV = np.ldexp(np.abs(A).astype(np.float64) @ dB, (e + f - 2 * p)[:, None]) + 40 * U * np.abs(V)
    s2 = np.sum(V * V, axis=0)
    d = 16 + 2 + 8 + NP // 512
    b = np.sum(2 * np.abs(V) * dV + dV * dV, axis=0) + (gamma(N + 1) + gamma(d)) * s2 + 2 * U * (c + noise)
    return b * (1 + 1e-9)                 # (the bound itself is computed in fp64)
