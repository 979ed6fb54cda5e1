// The two wave-level pieces of the pull-back (device units only): the mean-only pass over a model's sources and the damped
// Newton iteration around inv_pass / inv_solve (gpt_newton.h).  Shared by k_pullback_velocity (gpt_pullback.hip) and
// k_chain_velocity (gpt_chain.hip); every lane of the wave runs the same arithmetic on the same bits.
#pragma once
#include "gpt_common.h"
#include "gpt_exp.h"
#include "gpt_newton.h"

namespace gpt {

// f = mean of the model at x, the same in every lane.  qsc[d] = 1 / (sqrt(2) l_d).
template <int KT, int D>
__device__ __forceinline__ void pb_mean(const int N, const double lnc, const double* __restrict__ Xs, const double* __restrict__ A4,
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
#pragma unroll
        for (int d = 0; d < D; ++d) df[d] = xs[d] * RS2 - q[d];
        double hh = df[0] * df[0];
#pragma unroll
        for (int d = 1; d < D; ++d) hh = fma(df[d], df[d], hh);
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

// The iteration of k_inverse_newton (gpt_inverse.hip) from the start point in z, statement for statement — that kernel keeps its
// own loop so that its instruction stream stays what it was; both call the same inv_pass / inv_solve / inv_det.  On return z is
// the last accepted point, A = I + J(z) and rho = |z + mu(z) - y| there, passes the contractions over the sources spent;
// returns INV_*.  Every decision is wave-uniform and goes through readfirstlane, so the loop branches are scalar; no memory is
// touched between the passes.
template <int KT, int D>
__device__ __forceinline__ int pb_newton(const int N, const double lnc, const double* __restrict__ Xs, const double* __restrict__ A4,
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
            det = inv_det<D>(A);
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
