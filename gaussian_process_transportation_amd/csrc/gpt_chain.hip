// The transported policy through a chain of transports for gfx950 (MI355X): the reference's obstacle example
// (example/2D/surface_generalization_with_obstacle.py:142-200) moves a demonstration twice, from the old surface to the new one
// and then round an obstacle, Phi = Phi_1 o Phi_0, and refits a GP on the result; here the source dynamics f is pulled back
// through all K maps in one launch:  x = Phi^-1(y),  v(y) = J_Phi(x) f(x).
//
//  k_chain_velocity : one wave owns one query from start to end, four waves per workgroup, one launch, one barrier at entry for
//               the exp table.  With a guess x0 of the source-space preimage, a mean-only forward pass (inv_mean) through stages
//               0 .. K-2 gives every stage its start.  Then the stages are solved from the last to the first, each with the
//               damped Newton iteration of k_pullback_velocity (inv_newton, gpt_newton.h) on z + psi_k(z) = y_k and the
//               affine inverse x_k = gamma_k^-1(z_k), which is the y of the stage before; a stage that does not converge hands on
//               the point it reached.  f = the dynamics mean at x_0 and vel = B_{K-1} ... B_1 (A_0 (R_jac,0 f)), B_k = A_k
//               R_jac,k: the product of the outer stages is kept in registers as the sweep goes, the innermost stage is applied to
//               f in the association of k_pullback_velocity, so that K = 1 is that kernel's arithmetic.  Each stage's kernel
//               type and the dynamics' are wave-uniform run-time choices (scalar branches): the kernel is templated on D only.
//               Per-stage values are stored by lane 0 as each stage finishes; nothing is indexed by the run-time stage number
//               but the kernel arguments.  A query's sums run in a fixed order: its result does not depend on M or on the
//               queries around it.
//  k_chain_variance : one thread per query, plain fp64 FMA: the first-order propagation of each stage's Jacobian variance and
//               of the dynamics variance through the stages after it.
#include "gpt_chain_body.h"

namespace gpt {

template <int D>
__global__ __launch_bounds__(256) void k_chain_velocity(ChainArgs a) {
    __shared__ double Tt[256];
    Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
    __syncthreads();                                  // the only barrier: from here on the four waves of a workgroup are on their own
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    double y[D], x0[D], x[D], f[D], vel[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        y[d] = a.Y[m * D + d];
        x0[d] = a.X0 ? a.X0[m * D + d] : 0.0;
    }
    // the per-point body, shared with k_rollout (gpt_chain_body.h); per-stage values are stored by lane 0 as each stage finishes
    const int first = chain_point<D>(a.st, a.dyn, a.K, a.rtol, a.max_passes, Tt, lane, a.X0 != nullptr, x0, y, x, f, vel,
        [&](const int k, const double (&z)[D], const double (&xk)[D], const double (&A)[D][D], const int status, const int passes, const double rho) {
            if (lane != 0) return;
            const int64_t row = (int64_t)k * a.M + m;
#pragma unroll
            for (int o = 0; o < D; ++o) {
                if (a.stage_z) a.stage_z[row * D + o] = z[o];
                if (a.stage_x) a.stage_x[row * D + o] = xk[o];
                if (a.stage_A) {
#pragma unroll
                    for (int d = 0; d < D; ++d) a.stage_A[(row * D + o) * D + d] = A[o][d];
                }
            }
            if (a.stage_status) a.stage_status[row] = status;
            if (a.stage_passes) a.stage_passes[row] = passes;
            if (a.stage_residual) a.stage_residual[row] = rho;
            if (a.stage_det) a.stage_det[row] = sm_det<D>(A);
        });
    if (lane != 0) return;
#pragma unroll
    for (int o = 0; o < D; ++o) {
        a.vel[m * D + o] = vel[o];
        if (a.x) a.x[m * D + o] = x[o];
        if (a.f) a.f[m * D + o] = f[o];
    }
    a.status[m] = first;
}

template <int D>
__global__ __launch_bounds__(256) void k_chain_variance(ChainArgs a) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.M) return;
    const int K = a.K;
    // forward: v_{-1} = f, g_k = R_jac,k v_{k-1}, sigma_k^2 = sum_d Jvar_k[d] g_k[d]^2, v_k = A_k g_k
    double sig[CHAIN_MAX];                            // (unrolled: constants index it)
    if (a.vel_var_map) {
        double v[D];
#pragma unroll
        for (int i = 0; i < D; ++i) v[i] = a.f[m * D + i];
#pragma unroll
        for (int k = 0; k < CHAIN_MAX; ++k) {
            sig[k] = 0.0;
            if (k < K) {
                const double* Rj = a.st[k].R_jac;
                const int64_t row = (int64_t)k * a.M + m;
                double g[D], s = 0.0;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const double r = sm_row_dot<D>(Rj, i, v);
                    g[i] = r;
                    s = fma(a.stage_Jvar[row * D + i], r * r, s);
                }
                sig[k] = s;
                if (k + 1 < K) {
                    sm_mat_vec<D>(a.stage_A + row * D * D, g, v);
                }
            }
        }
    }
    // backward: Q = B_{K-1} ... B_{k+1} when stage k is reached, the whole product at the end
    double Q[D][D], acc[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        acc[i] = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) Q[i][d] = i == d ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = CHAIN_MAX - 1; k >= 0; --k) {
        if (k < K) {
            if (a.vel_var_map) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    double q2 = Q[i][0] * Q[i][0];
#pragma unroll
                    for (int d = 1; d < D; ++d) q2 = fma(Q[i][d], Q[i][d], q2);
                    acc[i] = fma(sig[k], q2, acc[i]);
                }
            }
            if (k == 0 && !a.vel_var_dyn) break;
            const double* Rj = a.st[k].R_jac;
            const int64_t row = (int64_t)k * a.M + m;
            double B[D][D], Qn[D][D];
#pragma unroll
            for (int o = 0; o < D; ++o)
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    double b = a.stage_A[(row * D + o) * D] * Rj[e];           // (A_k R_jac,k)[o][e]
#pragma unroll
                    for (int d = 1; d < D; ++d) b = fma(a.stage_A[(row * D + o) * D + d], Rj[d * D + e], b);
                    B[o][e] = b;
                }
#pragma unroll
            for (int o = 0; o < D; ++o)
#pragma unroll
                for (int e = 0; e < D; ++e) Qn[o][e] = sm_mat_el<D>(Q, B, o, e);
#pragma unroll
            for (int o = 0; o < D; ++o)
#pragma unroll
                for (int e = 0; e < D; ++e) Q[o][e] = Qn[o][e];
        }
    }
    if (a.vel_var_map) {
#pragma unroll
        for (int i = 0; i < D; ++i) a.vel_var_map[m * D + i] = acc[i];
    }
    if (a.vel_var_dyn) {
        const double sd = sqrt(a.var_dyn[m]) - a.std_offset, s2 = sd * sd;
#pragma unroll
        for (int o = 0; o < D; ++o) {
            double sum = 0.0;
#pragma unroll
            for (int e = 0; e < D; ++e) sum = fma(Q[o][e], Q[o][e], sum);
            a.vel_var_dyn[m * D + o] = s2 * sum;
        }
    }
}

void launch_chain_velocity(hipStream_t s, int D, const ChainArgs& a) {
    if (a.M <= 0) return;
    const dim3 grid((unsigned)((a.M + 3) / 4));           // one wave per query, four per workgroup (M < 2^31: the grid fits)
    with_small_dim(D, [&](auto d) { hipLaunchKernelGGL((k_chain_velocity<decltype(d)::value>), grid, dim3(256), 0, s, a); });
}

void launch_chain_variance(hipStream_t s, int D, const ChainArgs& a) {
    if (a.M <= 0 || !(a.vel_var_map || a.vel_var_dyn)) return;
    const dim3 grid((unsigned)((a.M + 255) / 256));
    with_small_dim(D, [&](auto d) { hipLaunchKernelGGL((k_chain_variance<decltype(d)::value>), grid, dim3(256), 0, s, a); });
}

}  // namespace gpt
