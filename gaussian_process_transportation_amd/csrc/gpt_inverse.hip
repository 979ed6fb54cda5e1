// Inverse of the displacement map for gfx950 (MI355X): solves  z + mu(z) = y  for M targets y in ONE launch, mu the posterior
// mean of a committed fp64 model with D == O <= 3 (the map of the reference's transport, policy_transportation.py:30-35, taken
// the other way: what example/2D/surface_generalization_heteroschedastic _inverse_mapping.py:88-127 approximates with a second
// fit and gaussian_process_transportation_diffeomorphic.py:109-121 measures the miss of).
//
//  k_inverse_newton : damped Newton.  One wave owns one query from its first pass to its last; every pass is the contraction
//               of k_mean_jac (gpt_predict.hip) at the current point — the 64 lanes stride the sources, the same scaled X and
//               A4 operands, 1/sqrt(2) scaling and exp2 table — reduced with the xor butterfly, after which EVERY lane holds
//               the same 1 + D sums per output, bit for bit.  Each lane then does the same D x D solve (adjugate) and takes
//               the same accept / reject decision; the decision goes through readfirstlane so that the loop branch is scalar.
//               No memory is touched between the passes; waves leave independently (one barrier, at entry, for the table).
//               A query's sums run in a fixed order (lane l takes sources l, l + 64, ..; butterfly 32, 16, .., 1): its result
//               does not depend on M or on the queries around it.
#include "gpt_common.h"
#include "gpt_exp.h"
#include "gpt_dispatch.h"
#include "gpt_newton.h"

namespace gpt {

template <int KT, int D>
__global__ __launch_bounds__(256) void k_inverse_newton(KernelParams p, const double* __restrict__ Xs, const double* __restrict__ A4,
                                                        InverseArgs a) {
    __shared__ double Tt[256];
    Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
    __syncthreads();                                  // the only barrier: from here on the four waves of a workgroup are on their own
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    const int N = p.N;
    const double lnc = p.lnc;
    double qsc[D], jsc[D], y[D], z[D], r[D], A[D][D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        qsc[d] = p.inv_ls[d] * 0.70710678118654752440;
        jsc[d] = p.inv_ls[d] * 1.41421356237309504880;
        y[d] = a.Y[m * D + d];
        z[d] = a.Z0 ? a.Z0[m * D + d] : y[d];
    }
    inv_pass<KT, D>(N, lnc, Xs, A4, Tt, lane, qsc, jsc, z, y, r, A);
    double rho = inv_norm<D>(r);
    const double tol = a.rtol * (1.0 + inv_norm<D>(y));
    double t = 1.0;
    int passes = 1, status;
    for (;;) {
        double det = 0.0;
        int stop = -1;
        if (rho <= tol) stop = INV_CONVERGED;
        else if (passes >= a.max_passes) stop = INV_MAX_PASSES;
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
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) a.Z[m * D + d] = z[d];
        if (a.residual) a.residual[m] = rho;
        if (a.det) a.det[m] = inv_det<D>(A);
        if (a.passes) a.passes[m] = passes;
        a.status[m] = status;
    }
}

void launch_inverse_newton(hipStream_t s, const KernelParams& p, const double* Xs, const double* A4, const InverseArgs& a) {
    if (a.M <= 0) return;
    const dim3 grid((unsigned)((a.M + 3) / 4));           // one wave per query, four per workgroup (M < 2^31: the grid fits)
    with_kernel_type(p.ktype, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if constexpr (KT != KT_MATERN12) {                 // (no derivative: the API refuses Matern 1/2 before a launch is reached)
            auto go = [&](auto d) { hipLaunchKernelGGL((k_inverse_newton<KT, decltype(d)::value>), grid, dim3(256), 0, s, p, Xs, A4, a); };
            switch (p.D) {
                case 1: go(Int<1>{}); break;
                case 2: go(Int<2>{}); break;
                default: go(Int<3>{});
            }
        }
    });
}

}  // namespace gpt
