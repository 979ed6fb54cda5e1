// Whole paths of the variance-stabilised policy for gfx950 (MI355X): the step of gpt_rollout_stab.h inside the loop of k_rollout.
// The reference integrates pos += mean - std * grad_var / |grad_var| on the host, 1000 steps (plot_traj_evolution); its variance
// and variance gradient are one triangular product with the inverse factor W per point, which is the work of this kernel.
//
//  k_rollout_stab : one workgroup of four waves owns four trajectories.  The per-point body (the K Newton inversions and the
//               dynamics mean of gpt_chain_body.h) is one wave's work per trajectory, as in k_rollout; the product with W is the
//               workgroup's joint work.  A step:
//                 1. body      each live wave: x_t = Phi^-1(y_t) (chain_invert; K = 0: x_t = y_t) and f_t = mean(x_t)
//                 2. B image   each wave writes the four columns k*, d_0 k*, d_1 k*, d_2 k* of its trajectory for every source
//                              into an NP x 16 image in LDS (trajectory j of the workgroup: columns 4j .. 4j+3; rows >= N, the
//                              columns of an ended trajectory and of a wave past M: zero).  One lane per source row, k and g
//                              from one exp (gpt_exp.h), the column formulas of k_var's generating sweep.
//                 3. sweep     after a barrier the four waves sweep Wf with v_mfma_f64_16x16x4_f64 (rollout_w_sweep of
//                              gpt_rollout_body.h: the deal of the 64-row groups, the layout of Wf, the prefetch): sixteen columns
//                              are one MFMA tile, so four trajectories fill the instruction one alone would use a quarter of.  The
//                              finished C tiles are squared and cross-multiplied with their k* column (the shuffle of k_var) into
//                              two sums per lane.
//                 4. reduce    across the lanes (two shuffles), then across the waves through LDS in wave order; a wave reads the
//                              four sums of its own columns.  MFMA columns do not mix and every order is fixed by N alone: a
//                              trajectory's var and gradient do not depend on its neighbours, alive or ended, nor on which of
//                              the four column groups it sits in.
//                 5. finish    each live wave: var, g, s, ghat, fs (gpt_rollout_stab.h), the push-forward (chain_push), the
//                              Euler step, the step's rows (lane 0), the end rule of k_rollout.
//               Entering a launch, the NaN rows after an end and leaving: gpt_rollout_body.h, as k_rollout.
//               Three barriers per step would be one too many: whether any trajectory is alive is read after the barrier of
//               step 2 from flags the waves set in step 5 of the step before, so a workgroup leaves together, one (empty) image
//               late.  Waves whose trajectory has ended keep writing zeros, sweeping and meeting the barriers until then.
#include "gpt_rollout_stab.h"
#include "gpt_rollout_body.h"
#include "gpt_chain_body.h"
#include "gpt_dispatch.h"

namespace gpt {

// Step 2: this wave's four columns of the B image, `col` = image + 4 w.  The distances, the kernel value and the derivative
// factor are the wave-level passes' own (gpt_newton.h: inv_diffs, inv_kernel_kg), which are k_var's D <= 3 generating sweep's:
// k* = c k, d_d k* = c g (sqrt2 / l_d) df_d, with g = k for RBF; columns of coordinates the model does not have are zero.
template <int KT, int D>
__device__ __forceinline__ void stab_columns(const ChainModel& m, const int NP, const double* __restrict__ Tt, const int lane,
                                             const bool live, const double (&x)[D], double* __restrict__ col) {
    double q[D], cd[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        q[d] = x[d] * (m.inv_ls[d] * 0.70710678118654752440);
        cd[d] = m.inv_ls[d] * 1.41421356237309504880;
    }
    for (int n = lane; n < NP; n += 64) {
        d4 b{0.0, 0.0, 0.0, 0.0};
        if (live && n < m.N) {
            double df[D], gv;
            const double hh = inv_diffs<D>(*reinterpret_cast<const d4*>(m.Xs + (size_t)n * 4), q, df);
            b[0] = inv_kernel_kg<KT>(hh, m.lnc, Tt, gv);
#pragma unroll
            for (int d = 0; d < D; ++d) b[1 + d] = gv * (cd[d] * df[d]);
        }
        *reinterpret_cast<d4*>(col + (size_t)n * 16) = b;
    }
}

// Step 3: this wave's share of V = W B (rollout_w_sweep), folded into ssq = sum of squares and crs = sum of products with the k*
// column of the lane's column (lane & 15), over the rows the lane holds.
__device__ __forceinline__ void stab_sweep(const double* __restrict__ Wf, const int N, const double* __restrict__ img, const int w,
                                           const int lane, double& ssq, double& crs) {
    ssq = 0.0; crs = 0.0;
    rollout_w_sweep(Wf, N, img, w, lane, [&](int, const d4 (&acc)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double v = acc[r][e];
                ssq += v * v;
                crs += v * __shfl(v, lane & ~3);
            }
    });
}

template <int D>
__global__ __launch_bounds__(256) void k_rollout_stab(RolloutStabArgs s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char img_raw[];      // the B image: NP x 16 doubles
    double* const img = reinterpret_cast<double*>(img_raw);
    __shared__ double Tt[256];
    __shared__ double red[4][2][16];                  // [wave][ssq | crs][column]
    __shared__ int live[4];                           // trajectory of wave w alive
    const RolloutArgs& a = s.r;
    Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t m = (int64_t)blockIdx.x * 4 + w;
    const int T = a.T, t_begin = a.t_begin, t_end = a.t_end;
    const bool entered = rollout_enters(a, m);
    bool alive = entered;
    RolloutCarry<D> c{};
    c.have_guess = true;
    if (alive) c = rollout_entry<D>(a, m, lane == 0);
    if (lane == 0) live[w] = alive ? 1 : 0;
    __syncthreads();
    int status = INV_CONVERGED, t_stop = t_end;
    for (int t = t_begin; t < t_end; ++t) {
        // ---- 1. body
        double x[D], f[D], Q[D][D], A[D][D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            x[i] = 0.0; f[i] = 0.0;
#pragma unroll
            for (int d = 0; d < D; ++d) { Q[i][d] = 0.0; A[i][d] = 0.0; }
        }
        if (alive) {
            if (a.K == 0) {
#pragma unroll
                for (int d = 0; d < D; ++d) x[d] = c.y[d];
            } else {
                status = chain_invert<D>(a.st, a.K, a.rtol, a.max_passes, Tt, lane, c.have_guess, c.guess, c.y, x, Q, A,
                                         [](int, const double (&)[D], const double (&)[D], const double (&)[D][D], int, int, double) {});
            }
            ch_mean<D>(a.dyn, Tt, lane, x, f);
        }
        // ---- 2. B image
        switch (a.dyn.ktype) {                        // (no Matern 1/2: the entry points refuse such a dynamics)
            case KT_MATERN32: stab_columns<KT_MATERN32, D>(a.dyn, s.NP, Tt, lane, alive, x, img + 4 * w); break;
            case KT_MATERN52: stab_columns<KT_MATERN52, D>(a.dyn, s.NP, Tt, lane, alive, x, img + 4 * w); break;
            default: stab_columns<KT_RBF, D>(a.dyn, s.NP, Tt, lane, alive, x, img + 4 * w);
        }
        __syncthreads();
        if (!(live[0] | live[1] | live[2] | live[3])) break;      // (the same for all four waves: set before the barrier above)
        // ---- 3. sweep
        double ssq, crs;
        stab_sweep(s.Wf, a.dyn.N, img, w, lane, ssq, crs);
        // ---- 4. reduce: rows of a column are spread over the 4 lane groups and over the 4 waves
        ssq += __shfl_xor(ssq, 16); ssq += __shfl_xor(ssq, 32);
        crs += __shfl_xor(crs, 16); crs += __shfl_xor(crs, 32);
        if (lane < 16) { red[w][0][lane] = ssq; red[w][1][lane] = crs; }
        __syncthreads();
        if (!alive) continue;
        // ---- 5. finish
        auto total = [&](const int which, const int col) { return ((red[0][which][col] + red[1][which][col]) + red[2][which][col]) + red[3][which][col]; };
        double var = s.c + s.noise - total(0, 4 * w);
        var = var < 0.0 ? 0.0 : var;
        double g[D], ghat[D], fs[D], vel[D], yn[D];
#pragma unroll
        for (int d = 0; d < D; ++d) g[d] = -2.0 * total(1, 4 * w + 1 + d);
        const double sd = sqrt(var) - s.std_offset;
        unit_gradient<D>(g, ghat);
#pragma unroll
        for (int d = 0; d < D; ++d) fs[d] = stabilised(f[d], s.gain, sd, ghat[d]);
        if (a.K == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) vel[d] = fs[d];
        } else {
            chain_push<D>(a.st, a.K, Q, A, fs, vel);
        }
        bool ok = status == INV_CONVERGED;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            yn[d] = euler_step(c.y[d], a.dt, vel[d]);
            ok = ok && __builtin_isfinite(yn[d]);
        }
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (a.vel) step_row<D>(a, a.vel, m, t)[d] = vel[d];
                if (a.x) step_row<D>(a, a.x, m, t)[d] = x[d];
                if (s.f) step_row<D>(a, s.f, m, t)[d] = f[d];
                if (s.dvar) step_row<D>(a, s.dvar, m, t)[d] = g[d];
            }
            if (s.var) s.var[m * (int64_t)T + t] = var;
        }
        if (__builtin_amdgcn_readfirstlane(ok ? 1 : 0)) {      // (every lane holds the same value)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (lane == 0) path_row<D>(a, m, (int64_t)t + 1)[d] = yn[d];
                c.y[d] = yn[d];
                c.guess[d] = x[d];
            }
            c.have_guess = true;
        } else {                                      // ended at step t: nothing after it exists
            alive = false;
            t_stop = t;
            if (lane == 0) live[w] = 0;
            rollout_end_fill<D>(a, RolloutOwn{{s.f, s.dvar}, {s.var, nullptr}, nullptr}, m, t, lane);
        }
    }
    if (entered && lane == 0) rollout_leave<D>(a, m, t_stop, status, alive, c.guess);
}

void launch_rollout_stab(hipStream_t st, int D, const RolloutStabArgs& a) {
    if (a.r.M <= 0) return;
    const dim3 grid((unsigned)((a.r.M + 3) / 4));         // four trajectories per workgroup (M < 2^31: the grid fits)
    // (the image of the largest admitted model, whatever NP is: launch_lds opts a kernel into one size, once per device)
    constexpr size_t lds = (size_t)ROLLOUT_STAB_MAX_N * 16 * sizeof(double);
    with_small_dim(D, [&](auto d) { launch_lds<k_rollout_stab<decltype(d)::value>>(grid, dim3(256), lds, st, a); });
}

}  // namespace gpt
