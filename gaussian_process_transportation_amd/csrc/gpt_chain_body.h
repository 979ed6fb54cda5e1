// One target-space point through a chain of transports inside one wave (device units only): the body of k_chain_velocity
// (gpt_chain.hip), which k_rollout (gpt_rollout.hip) runs once per time step.  Every lane of the wave runs the same arithmetic on
// the same bits (gpt_newton.h), so every value below is the same in every lane; what a kernel stores, its lane 0 stores.
#pragma once
#include "gpt_chain.h"
#include "gpt_newton.h"

namespace gpt {

// f = mean of the model at x; the kernel type is the same in every wave of the launch
template <int D>
__device__ __forceinline__ void ch_mean(const ChainModel& m, const double* __restrict__ Tt, const int lane, const double (&x)[D],
                                        double (&f)[D]) {
    double qsc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) qsc[d] = m.inv_ls[d] * 0.70710678118654752440;
    switch (m.ktype) {
        case KT_MATERN12: inv_mean<KT_MATERN12, D>(m.N, m.lnc, m.Xs, m.A4, Tt, lane, qsc, x, f); break;
        case KT_MATERN32: inv_mean<KT_MATERN32, D>(m.N, m.lnc, m.Xs, m.A4, Tt, lane, qsc, x, f); break;
        case KT_MATERN52: inv_mean<KT_MATERN52, D>(m.N, m.lnc, m.Xs, m.A4, Tt, lane, qsc, x, f); break;
        default: inv_mean<KT_RBF, D>(m.N, m.lnc, m.Xs, m.A4, Tt, lane, qsc, x, f);
    }
}

// The first half of chain_point: x = Phi^-1(y) for 1 <= K <= CHAIN_MAX stages `st` (the
// kernel's arguments: the only thing a run-time stage number indexes).  With `guess` (wave-uniform), x0 is a guess of the
// source-space preimage: a mean-only forward pass through stages 0 .. K-2 gives every stage its start; without it every stage
// starts at its own y_k (x0 is not read).  The stages are solved from the last to the first, each with the damped Newton iteration
// of k_pullback_velocity on z + psi_k(z) = y_k and the affine inverse x_k = gamma_k^-1(z_k), the y of the stage before; a stage
// that does not converge hands on the point it reached.  Q, the product B_{K-1} ... B_1 of the outer stages (B_k = A_k R_jac,k; the
// identity for K = 1), is kept in registers as the sweep goes; A is left as stage 0's, for chain_push.
// stage(k, z, x_k, A, status, passes, rho) is called as each stage finishes.  Returns the INV_* of the first stage in solve
// order that is not CONVERGED, else CONVERGED.
template <int D, class Stage>
__device__ __forceinline__ int chain_invert(const ChainStage (&st)[CHAIN_MAX], const int K, const double rtol,
                                            const int max_passes, const double* __restrict__ Tt, const int lane, const bool guess,
                                            const double (&x0)[D], const double (&y_in)[D], double (&x)[D], double (&Q)[D][D],
                                            double (&A)[D][D], Stage&& stage) {
    double y[D];
    double start[CHAIN_MAX][D];                       // only ever indexed by unrolled constants: registers
#pragma unroll
    for (int k = 0; k < CHAIN_MAX; ++k)
#pragma unroll
        for (int d = 0; d < D; ++d) start[k][d] = 0.0;
    if (guess) {                                      // g_0 = x0; stage k starts at gamma_k(g_k); g_{k+1} = gamma_k(g_k) + mean_k(gamma_k(g_k))
        double g[D];
#pragma unroll
        for (int d = 0; d < D; ++d) g[d] = x0[d];
        for (int k = 0; k < K; ++k) {
            double z0[D];
            sm_affine<D>(st[k], st[k].R, g, z0);         // the arithmetic of k_affine (gpt_transport.hip)
#pragma unroll
            for (int j = 0; j < CHAIN_MAX; ++j)
                if (j == k) {
#pragma unroll
                    for (int d = 0; d < D; ++d) start[j][d] = z0[d];
                }
            if (k + 1 < K) {
                double mu[D];
                ch_mean<D>(st[k].m, Tt, lane, z0, mu);
#pragma unroll
                for (int d = 0; d < D; ++d) g[d] = z0[d] + mu[d];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
        y[i] = y_in[i];
        x[i] = y[i];
#pragma unroll
        for (int d = 0; d < D; ++d) Q[i][d] = i == d ? 1.0 : 0.0;
    }
    int first = INV_CONVERGED;
    for (int k = K - 1; k >= 0; --k) {
        const ChainStage& S = st[k];
        double R[D][D], qsc[D], jsc[D], z[D], rho;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int d = 0; d < D; ++d) R[i][d] = S.R[i * D + d];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            qsc[d] = S.m.inv_ls[d] * 0.70710678118654752440;
            jsc[d] = S.m.inv_ls[d] * 1.41421356237309504880;
            z[d] = y[d];
        }
        if (guess) {
#pragma unroll
            for (int j = 0; j < CHAIN_MAX; ++j)
                if (j == k) {
#pragma unroll
                    for (int d = 0; d < D; ++d) z[d] = start[j][d];
                }
        }
        int passes, status;
        switch (S.m.ktype) {                          // (no Matern 1/2: the API refuses such a stage before a launch is reached)
            case KT_MATERN32:
                status = inv_newton<KT_MATERN32, D>(S.m.N, S.m.lnc, S.m.Xs, S.m.A4, Tt, lane, qsc, jsc, y, rtol, max_passes, z, A, rho, passes);
                break;
            case KT_MATERN52:
                status = inv_newton<KT_MATERN52, D>(S.m.N, S.m.lnc, S.m.Xs, S.m.A4, Tt, lane, qsc, jsc, y, rtol, max_passes, z, A, rho, passes);
                break;
            default:
                status = inv_newton<KT_RBF, D>(S.m.N, S.m.lnc, S.m.Xs, S.m.A4, Tt, lane, qsc, jsc, y, rtol, max_passes, z, A, rho, passes);
        }
        if (first == INV_CONVERGED) first = status;
        // x = (z - c_dst) R / scale + c_src, the arithmetic of k_pullback_velocity
        double zc[D];
#pragma unroll
        for (int d = 0; d < D; ++d) zc[d] = z[d] - S.c_dst[d];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double r = sm_col_dot<D>(zc, R, i);
            x[i] = r / S.scale + S.c_src[i];
        }
        stage(k, z, x, A, status, passes, rho);
        if (k > 0) {                                  // Q <- Q (A_k R_jac,k); the innermost stage is applied to f below
            double B[D][D], Qn[D][D];
#pragma unroll
            for (int o = 0; o < D; ++o)
#pragma unroll
                for (int e = 0; e < D; ++e) {
                    double b = A[o][0] * S.R_jac[e];
#pragma unroll
                    for (int d = 1; d < D; ++d) b = fma(A[o][d], S.R_jac[d * D + e], b);
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
#pragma unroll
            for (int d = 0; d < D; ++d) y[d] = x[d];
        }
    }
    return first;
}

// The second half: vel = Q (A_0 (R_jac,0 f)) for a source-space vector f at the x chain_invert found (Q and A as it left them).  The
// innermost stage is applied to f in the association of k_pullback_velocity, so that K = 1 is that kernel's arithmetic.
template <int D>
__device__ __forceinline__ void chain_push(const ChainStage (&st)[CHAIN_MAX], const int K, const double (&Q)[D][D],
                                           const double (&A)[D][D], const double (&f)[D], double (&vel)[D]) {
    double g[D], h[D];
    const double* Rj = st[0].R_jac;
#pragma unroll
    for (int i = 0; i < D; ++i) g[i] = sm_row_dot<D>(Rj, i, f);
#pragma unroll
    for (int o = 0; o < D; ++o) {
        double r = A[o][0] * g[0];
#pragma unroll
        for (int d = 1; d < D; ++d) r = fma(A[o][d], g[d], r);
        h[o] = r;
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
        double r = h[o];
        if (K > 1) {                                  // (Q = I otherwise: nothing to multiply, and no 0 * inf of a point that ran away)
            r = Q[o][0] * h[0];
#pragma unroll
            for (int d = 1; d < D; ++d) r = fma(Q[o][d], h[d], r);
        }
        vel[o] = r;
    }
}

// x = Phi^-1(y), f = the dynamics mean at x, vel = B_{K-1} ... B_1 (A_0 (R_jac,0 f)): chain_invert, the mean, chain_push.
template <int D, class Stage>
__device__ __forceinline__ int chain_point(const ChainStage (&st)[CHAIN_MAX], const ChainModel& dyn, const int K, const double rtol,
                                           const int max_passes, const double* __restrict__ Tt, const int lane, const bool guess,
                                           const double (&x0)[D], const double (&y_in)[D], double (&x)[D], double (&f)[D],
                                           double (&vel)[D], Stage&& stage) {
    double Q[D][D], A[D][D];
    const int first = chain_invert<D>(st, K, rtol, max_passes, Tt, lane, guess, x0, y_in, x, Q, A, stage);
    ch_mean<D>(dyn, Tt, lane, x, f);
    chain_push<D>(st, K, Q, A, f, vel);
    return first;
}

}  // namespace gpt
