// The transported policy at target-space points for gfx950 (MI355X): what a user of the reference does after transporting a
// demonstration — evaluate the moved dynamics at a point y of the new scene that is not on it.  The reference refits a second
// GP on the moved demonstration (example/2D/surface_generalization.py:81-88) and a third for the uncertainty
// (surface_generalization_heteroschedastic_uncertainty.py:150-175); here the source dynamics f is pulled back through the
// transport Phi = gamma + psi o gamma itself:  x = Phi^-1(y),  v(y) = J_Phi(x) f(x).
//
//  k_pullback_velocity : one wave owns one query from its first pass to its last, four waves per workgroup, one launch.
//               z: the damped Newton iteration of k_inverse_newton (the same inv_pass / inv_solve, gpt_newton.h) on
//               z + psi(z) = y from gamma(x0) or y; x = gamma^-1(z); f = the dynamics mean at x, a mean-only pass of the same shape as Newton's (the 64
//               lanes stride the sources, Xs / A4 rows of 4, 1/sqrt(2) scaling, table exp, xor butterfly: every lane holds the
//               same bits) over the SECOND model's blob; vel = A R_jac f with A = I + J_psi(z) of the last accepted pass.  The
//               short algebra is done redundantly per lane and stored by lane 0.  One barrier, at entry, for the table; no
//               memory is touched between passes; a query's sums run in a fixed order, so its result does not depend on M or
//               on the queries around it.
//  k_pullback_variance : one thread per query, plain fp64 FMA: the two variances of vel from the variance launches' outputs.
#include "gpt_pullback.h"
#include "gpt_newton.h"

namespace gpt {

template <int KT_MAP, int KT_DYN, int D>
__global__ __launch_bounds__(256) void k_pullback_velocity(KernelParams pm, const double* __restrict__ Xs_map, const double* __restrict__ A4_map,
                                                           KernelParams pd, const double* __restrict__ Xs_dyn,
                                                           const double* __restrict__ A4_dyn, PullbackArgs a) {
    __shared__ double Tt[256];
    Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
    __syncthreads();                                  // the only barrier: from here on the four waves of a workgroup are on their own
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    double R[D][D], qsc[D], jsc[D], y[D], z[D], A[D][D], rho;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int d = 0; d < D; ++d) R[i][d] = a.R[i * D + d];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        qsc[d] = pm.inv_ls[d] * 0.70710678118654752440;
        jsc[d] = pm.inv_ls[d] * 1.41421356237309504880;
        y[d] = a.Y[m * D + d];
        z[d] = y[d];
    }
    if (a.X0) sm_affine<D>(a, R, a.X0 + m * D, z);     // gamma(x0), the arithmetic of k_affine (gpt_transport.hip)
    int passes;
    const int status = inv_newton<KT_MAP, D>(pm.N, pm.lnc, Xs_map, A4_map, Tt, lane, qsc, jsc, y, a.rtol, a.max_passes, z, A, rho, passes);
    // x = (z - c_dst) R / scale + c_src.  Written out, where k_chain_velocity (gpt_chain.hip) calls sm_col_dot for the same sum:
    // with the helper here the compiler commutes the final addition, and this kernel's instructions are to stay what they were
    double x[D], f[D], g[D], zc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) zc[d] = z[d] - a.c_dst[d];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double r = zc[0] * R[0][i];
#pragma unroll
        for (int d = 1; d < D; ++d) r = fma(zc[d], R[d][i], r);
        x[i] = r / a.scale + a.c_src[i];
    }
#pragma unroll
    for (int d = 0; d < D; ++d) qsc[d] = pd.inv_ls[d] * 0.70710678118654752440;
    inv_mean<KT_DYN, D>(pd.N, pd.lnc, Xs_dyn, A4_dyn, Tt, lane, qsc, x, f);
    if (lane != 0) return;
    // vel = A (R_jac f)
    sm_mat_vec<D>(a.R_jac, f, g);
#pragma unroll
    for (int o = 0; o < D; ++o) {
        a.vel[m * D + o] = sm_row_dot<D>(A, o, g);
        if (a.x) a.x[m * D + o] = x[o];
        if (a.z) a.z[m * D + o] = z[o];
        if (a.f) a.f[m * D + o] = f[o];
        if (a.A) {
#pragma unroll
            for (int d = 0; d < D; ++d) a.A[(m * D + o) * D + d] = A[o][d];
        }
    }
    if (a.residual) a.residual[m] = rho;
    if (a.det) a.det[m] = sm_det<D>(A);
    if (a.passes) a.passes[m] = passes;
    a.status[m] = status;
}

template <int D>
__global__ __launch_bounds__(256) void k_pullback_variance(PullbackArgs a) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.M) return;
    double Rj[D][D], f[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        f[i] = a.f[m * D + i];
#pragma unroll
        for (int d = 0; d < D; ++d) Rj[i][d] = a.R_jac[i * D + d];
    }
    if (a.vel_var_map) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double g = sm_row_dot<D>(Rj, i, f);
            v = fma(a.Jvar[m * D + i], g * g, v);
        }
        a.vel_var_map[m] = v;
    }
    if (a.vel_var_dyn) {
        const double sd = sqrt(a.var_dyn[m]) - a.std_offset, s2 = sd * sd;
#pragma unroll
        for (int o = 0; o < D; ++o) {
            double sum = 0.0;
#pragma unroll
            for (int e = 0; e < D; ++e) {
                const double b = sm_mat_el<D>(a.A + m * D * D, Rj, o, e);     // (A R_jac)[o][e]
                sum = fma(b, b, sum);
            }
            a.vel_var_dyn[m * D + o] = s2 * sum;
        }
    }
}

void launch_pullback_velocity(hipStream_t s, const KernelParams& pm, const double* Xs_map, const double* A4_map, const KernelParams& pd,
                              const double* Xs_dyn, const double* A4_dyn, const PullbackArgs& a) {
    if (a.M <= 0) return;
    const dim3 grid((unsigned)((a.M + 3) / 4));           // one wave per query, four per workgroup (M < 2^31: the grid fits)
    with_kernel_type(pm.ktype, [&](auto km) {
        constexpr int KM = decltype(km)::value;
        if constexpr (KM != KT_MATERN12) {                 // (no derivative: the API refuses a Matern 1/2 map before a launch is reached)
            with_kernel_type(pd.ktype, [&](auto kd) {
                constexpr int KD = decltype(kd)::value;
                with_small_dim(pm.D, [&](auto d) {
                    hipLaunchKernelGGL((k_pullback_velocity<KM, KD, decltype(d)::value>), grid, dim3(256), 0, s, pm, Xs_map, A4_map, pd, Xs_dyn,
                                       A4_dyn, a);
                });
            });
        }
    });
}

void launch_pullback_variance(hipStream_t s, int D, const PullbackArgs& a) {
    if (a.M <= 0 || !(a.vel_var_map || a.vel_var_dyn)) return;
    const dim3 grid((unsigned)((a.M + 255) / 256));
    with_small_dim(D, [&](auto d) { hipLaunchKernelGGL((k_pullback_variance<decltype(d)::value>), grid, dim3(256), 0, s, a); });
}

}  // namespace gpt
