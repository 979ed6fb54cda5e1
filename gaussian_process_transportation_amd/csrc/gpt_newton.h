// Damped Newton on  z + mu(z) = y  inside one wave (device units only): the pass over the sources, the D x D solve and the
// iteration around them, and the mean-only pass; shared by k_inverse_newton (gpt_inverse.hip), k_pullback_velocity
// (gpt_pullback.hip) and k_chain_velocity (gpt_chain.hip).  Every lane of the wave runs the same arithmetic on the same bits;
// what differs between lanes is the stride of sources a lane sums before the xor butterfly.  mu: the posterior mean of a
// committed fp64 model with D == O <= 3.
#pragma once
#include "gpt_common.h"
#include "gpt_exp.h"
#include "gpt_small.h"

namespace gpt {

// s = adj(A) r / det
template <int D> __device__ __forceinline__ void inv_solve(const double (&A)[D][D], const double det, const double (&r)[D], double (&s)[D]) {
    const double id = 1.0 / det;
    if constexpr (D == 1) s[0] = r[0] * id;
    else if constexpr (D == 2) {
        s[0] = (A[1][1] * r[0] - A[0][1] * r[1]) * id;
        s[1] = (A[0][0] * r[1] - A[1][0] * r[0]) * id;
    } else {
        s[0] = ((A[1][1] * A[2][2] - A[1][2] * A[2][1]) * r[0] + (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * r[1] +
                (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * r[2]) * id;
        s[1] = ((A[1][2] * A[2][0] - A[1][0] * A[2][2]) * r[0] + (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * r[1] +
                (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * r[2]) * id;
        s[2] = ((A[1][0] * A[2][1] - A[1][1] * A[2][0]) * r[0] + (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * r[1] +
                (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * r[2]) * id;
    }
}

template <int D> __device__ __forceinline__ double inv_norm(const double (&v)[D]) {
    double s = v[0] * v[0];
#pragma unroll
    for (int d = 1; d < D; ++d) s = fma(v[d], v[d], s);
    return sqrt(s);
}

// One source against one point, as every wave-level pass and the B image of k_rollout_stab (gpt_rollout_stab.hip) take it: the source row
// xs carries X / l, the point q = x / (sqrt2 l); df_d = X_d / (sqrt2 l_d) - q_d and the return value h = |df|^2 = r^2 / 2.
template <int D> __device__ __forceinline__ double inv_diffs(const d4& xs, const double (&q)[D], double (&df)[D]) {
    constexpr double RS2 = 0.70710678118654752440;
#pragma unroll
    for (int d = 0; d < D; ++d) df[d] = xs[d] * RS2 - q[d];
    double hh = df[0] * df[0];
#pragma unroll
    for (int d = 1; d < D; ++d) hh = fma(df[d], df[d], hh);
    return hh;
}
// c k (returned) and c g (gpt_exp.h: the factor of a derivative, d k / d x_d = c g (sqrt2 / l_d) df_d; g = k for RBF) from h
template <int KT> __device__ __forceinline__ double inv_kernel_kg(const double hh, const double lnc, const double* __restrict__ Tt, double& gv) {
    double kv;
    if constexpr (KT == KT_MATERN32 || KT == KT_MATERN52) kv = kernel_tab_kg<KT>(hh, lnc, Tt, gv);     // c k and c g from one exp
    else { kv = kernel_tab<KT>(hh, lnc, Tt); gv = kv; }
    return kv;
}

// One pass: r = z + mu(z) - y and A = I + J(z), the same in every lane.  qsc[d] = 1 / (sqrt(2) l_d), jsc[d] = sqrt(2) / l_d.
template <int KT, int D>
__device__ __forceinline__ void inv_pass(const int N, const double lnc, const double* __restrict__ Xs, const double* __restrict__ A4,
                                         const double* __restrict__ Tt, const int lane, const double (&qsc)[D], const double (&jsc)[D],
                                         const double (&z)[D], const double (&y)[D], double (&r)[D], double (&A)[D][D]) {
    constexpr double RS2 = 0.70710678118654752440;
    double q[D], acc[D][1 + D];
#pragma unroll
    for (int d = 0; d < D; ++d) q[d] = z[d] * qsc[d];
#pragma unroll
    for (int o = 0; o < D; ++o)
#pragma unroll
        for (int e = 0; e < 1 + D; ++e) acc[o][e] = 0.0;
#pragma unroll 2
    for (int n = lane; n < N; n += 64) {
        const d4 xs = *reinterpret_cast<const d4*>(Xs + (size_t)n * 4);
        const d4 al = *reinterpret_cast<const d4*>(A4 + (size_t)n * 4);
        double df[D], gv;
        const double hh = inv_diffs<D>(xs, q, df);
        const double kv = inv_kernel_kg<KT>(hh, lnc, Tt, gv);
#pragma unroll
        for (int o = 0; o < D; ++o) {
            acc[o][0] += kv * al[o];
            const double tg = gv * al[o];
#pragma unroll
            for (int d = 0; d < D; ++d) acc[o][1 + d] += tg * df[d];
        }
    }
#pragma unroll
    for (int o = 0; o < D; ++o)
#pragma unroll
        for (int e = 0; e < 1 + D; ++e) {
            double v = acc[o][e];
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);     // a + b on one side, b + a on the other: the same bits in every lane
            acc[o][e] = v;
        }
#pragma unroll
    for (int o = 0; o < D; ++o) {
        r[o] = z[o] + acc[o][0] - y[o];
#pragma unroll
        for (int d = 0; d < D; ++d) A[o][d] = (o == d ? 1.0 : 0.0) + acc[o][1 + d] * jsc[d];
    }
}

// f = mean of the model at x, the same in every lane.  qsc[d] = 1 / (sqrt(2) l_d).
template <int KT, int D>
__device__ __forceinline__ void inv_mean(const int N, const double lnc, const double* __restrict__ Xs, const double* __restrict__ A4,
                                        const double* __restrict__ Tt, const int lane, const double (&qsc)[D], const double (&x)[D],
                                        double (&f)[D]) {
    constexpr double RS2 = 0.70710678118654752440;
    double q[D], acc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { q[d] = x[d] * qsc[d]; acc[d] = 0.0; }
#pragma unroll 2
    for (int n = lane; n < N; n += 64) {
        const d4 xs = *reinterpret_cast<const d4*>(Xs + (size_t)n * 4);
        const d4 al = *reinterpret_cast<const d4*>(A4 + (size_t)n * 4);
        double df[D];
        const double hh = inv_diffs<D>(xs, q, df);
        const double kv = kernel_tab<KT>(hh, lnc, Tt);
#pragma unroll
        for (int o = 0; o < D; ++o) acc[o] += kv * al[o];
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
        double v = acc[o];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);         // the same bits in every lane
        f[o] = v;
    }
}

// The damped iteration from the start point in z.  On return z is
// the last accepted point, A = I + J(z) and rho = |z + mu(z) - y| there, passes the contractions over the sources spent;
// returns INV_*.  Every decision is wave-uniform and goes through readfirstlane, so the loop branches are scalar; no memory is
// touched between the passes.
template <int KT, int D>
__device__ __forceinline__ int inv_newton(const int N, const double lnc, const double* __restrict__ Xs, const double* __restrict__ A4,
                                          const double* __restrict__ Tt, const int lane, const double (&qsc)[D], const double (&jsc)[D],
                                          const double (&y)[D], const double rtol, const int max_passes, double (&z)[D],
                                          double (&A)[D][D], double& rho, int& passes) {
    double r[D];
    inv_pass<KT, D>(N, lnc, Xs, A4, Tt, lane, qsc, jsc, z, y, r, A);
    rho = inv_norm<D>(r);
    const double tol = rtol * (1.0 + inv_norm<D>(y));
    double t = 1.0;
    int status;
    passes = 1;
    for (;;) {
        double det = 0.0;
        int stop = -1;
        if (rho <= tol) stop = INV_CONVERGED;
        else if (passes >= max_passes) stop = INV_MAX_PASSES;
        else {
            det = sm_det<D>(A);
            double f2 = 0.0;
#pragma unroll
            for (int o = 0; o < D; ++o)
#pragma unroll
                for (int d = 0; d < D; ++d) f2 = fma(A[o][d], A[o][d], f2);
            const double fD = D == 1 ? sqrt(f2) : (D == 2 ? f2 : f2 * sqrt(f2));       // |A|_F^D
            if (fabs(det) <= 0x1p-40 * fD) stop = INV_SINGULAR;
        }
        status = __builtin_amdgcn_readfirstlane(stop);       // (every lane holds the same value; this tells the compiler so)
        if (status >= 0) break;
        double s[D], zn[D], rn[D], An[D][D];
        inv_solve<D>(A, det, r, s);
#pragma unroll
        for (int d = 0; d < D; ++d) zn[d] = z[d] - t * s[d];
        inv_pass<KT, D>(N, lnc, Xs, A4, Tt, lane, qsc, jsc, zn, y, rn, An);
        ++passes;
        const double rhon = inv_norm<D>(rn);
        const int accept = __builtin_amdgcn_readfirstlane(rhon < rho ? 1 : 0);     // (false for NaN; below a finite rho it is finite)
        if (accept) {
#pragma unroll
            for (int o = 0; o < D; ++o) {
                z[o] = zn[o]; r[o] = rn[o];
#pragma unroll
                for (int d = 0; d < D; ++d) A[o][d] = An[o][d];
            }
            rho = rhon;
            t = fmin(1.0, t + t);
        } else {
            t *= 0.5;
            const int stalled = __builtin_amdgcn_readfirstlane(t < 0x1p-20 ? 1 : 0);
            if (stalled) { status = INV_STALLED; break; }
        }
    }
    return status;
}

}  // namespace gpt
