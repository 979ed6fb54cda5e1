// Inverse of the displacement map for gfx950 (MI355X): solves  z + mu(z) = y  for M targets y in ONE launch, mu the posterior
// mean of a committed fp64 model with D == O <= 3 (the map of the reference's transport, policy_transportation.py:30-35, taken
// the other way: what example/2D/surface_generalization_heteroschedastic _inverse_mapping.py:88-127 approximates with a second
// fit and gaussian_process_transportation_diffeomorphic.py:109-121 measures the miss of).
//
//  k_inverse_newton : damped Newton (inv_newton, gpt_newton.h).  One wave owns one query from its first pass to its last; every pass is the contraction
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
    double qsc[D], jsc[D], y[D], z[D], A[D][D], rho;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        qsc[d] = p.inv_ls[d] * 0.70710678118654752440;
        jsc[d] = p.inv_ls[d] * 1.41421356237309504880;
        y[d] = a.Y[m * D + d];
        z[d] = a.Z0 ? a.Z0[m * D + d] : y[d];
    }
    int passes;
    const int status = inv_newton<KT, D>(N, lnc, Xs, A4, Tt, lane, qsc, jsc, y, a.rtol, a.max_passes, z, A, rho, passes);
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) a.Z[m * D + d] = z[d];
        if (a.residual) a.residual[m] = rho;
        if (a.det) a.det[m] = sm_det<D>(A);
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
            with_small_dim(p.D, [&](auto d) { hipLaunchKernelGGL((k_inverse_newton<KT, decltype(d)::value>), grid, dim3(256), 0, s, p, Xs, A4, a); });
        }
    });
}

}  // namespace gpt
