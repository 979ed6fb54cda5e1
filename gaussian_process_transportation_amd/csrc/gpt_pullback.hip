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
#include "gpt_dispatch.h"
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
    if (a.X0) {                                       // gamma(x0), the arithmetic of k_affine (gpt_transport.hip)
        double x0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x0[d] = a.X0[m * D + d] - a.c_src[d];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double r = R[i][0] * x0[0];
#pragma unroll
            for (int d = 1; d < D; ++d) r = fma(R[i][d], x0[d], r);
            z[i] = fma(a.scale, r, a.c_dst[i]);
        }
    }
    int passes;
    const int status = pb_newton<KT_MAP, D>(pm.N, pm.lnc, Xs_map, A4_map, Tt, lane, qsc, jsc, y, a.rtol, a.max_passes, z, A, rho, passes);
    // x = (z - c_dst) R / scale + c_src
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
    pb_mean<KT_DYN, D>(pd.N, pd.lnc, Xs_dyn, A4_dyn, Tt, lane, qsc, x, f);
    if (lane != 0) return;
    // vel = A (R_jac f)
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double r = a.R_jac[i * D] * f[0];
#pragma unroll
        for (int d = 1; d < D; ++d) r = fma(a.R_jac[i * D + d], f[d], r);
        g[i] = r;
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
        double r = A[o][0] * g[0];
#pragma unroll
        for (int d = 1; d < D; ++d) r = fma(A[o][d], g[d], r);
        a.vel[m * D + o] = r;
        if (a.x) a.x[m * D + o] = x[o];
        if (a.z) a.z[m * D + o] = z[o];
        if (a.f) a.f[m * D + o] = f[o];
        if (a.A) {
#pragma unroll
            for (int d = 0; d < D; ++d) a.A[(m * D + o) * D + d] = A[o][d];
        }
    }
    if (a.residual) a.residual[m] = rho;
    if (a.det) a.det[m] = inv_det<D>(A);
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
            double g = Rj[i][0] * f[0];
#pragma unroll
            for (int d = 1; d < D; ++d) g = fma(Rj[i][d], f[d], g);
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
                double b = a.A[(m * D + o) * D] * Rj[0][e];               // (A R_jac)[o][e]
#pragma unroll
                for (int d = 1; d < D; ++d) b = fma(a.A[(m * D + o) * D + d], Rj[d][e], b);
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
                auto go = [&](auto d) {
                    hipLaunchKernelGGL((k_pullback_velocity<KM, KD, decltype(d)::value>), grid, dim3(256), 0, s, pm, Xs_map, A4_map, pd, Xs_dyn,
                                       A4_dyn, a);
                };
                switch (pm.D) {
                    case 1: go(Int<1>{}); break;
                    case 2: go(Int<2>{}); break;
                    default: go(Int<3>{});
                }
            });
        }
    });
}

void launch_pullback_variance(hipStream_t s, int D, const PullbackArgs& a) {
    if (a.M <= 0 || !(a.vel_var_map || a.vel_var_dyn)) return;
    const dim3 grid((unsigned)((a.M + 255) / 256));
    auto go = [&](auto d) { hipLaunchKernelGGL((k_pullback_variance<decltype(d)::value>), grid, dim3(256), 0, s, a); };
    switch (D) {
        case 1: go(Int<1>{}); break;
        case 2: go(Int<2>{}); break;
        default: go(Int<3>{});
    }
}

}  // namespace gpt
