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
//                 3. sweep     after a barrier the four waves sweep Wf with v_mfma_f64_16x16x4_f64: sixteen columns are one
//                              MFMA tile, so four trajectories fill the instruction one alone would use a quarter of.  A wave
//                              takes whole 64-row groups (the 2 KiB records of k_pack_w, 16 bytes per lane), dealt 0 1 2 3 3 2 1 0
//                              per eight groups: the triangle gives group G 16 (G + 1) k4-steps, and this deal gives every wave
//                              the same number where round-robin would give the last wave twice the first's.  A row tile runs k
//                              to its diagonal only; row tiles >= N are skipped.  The finished C tile is squared and
//                              cross-multiplied with its k* column (the shuffle of k_var) into two sums per lane.
//                 4. reduce    across the lanes (two shuffles), then across the waves through LDS in wave order; a wave reads the
//                              four sums of its own columns.  MFMA columns do not mix and every order is fixed by N alone: a
//                              trajectory's var and gradient do not depend on its neighbours, alive or ended, nor on which of
//                              the four column groups it sits in.
//                 5. finish    each live wave: var, g, s, ghat, fs (gpt_rollout_stab.h), the push-forward (chain_push), the
//                              Euler step, the step's rows (lane 0), the end rule of k_rollout.
//               Three barriers per step would be one too many: whether any trajectory is alive is read after the barrier of
//               step 2 from flags the waves set in step 5 of the step before, so a workgroup leaves together, one (empty) image
//               late.  Waves whose trajectory has ended keep writing zeros, sweeping and meeting the barriers until then.
#include "gpt_rollout_stab.h"
#include "gpt_chain_body.h"
#include "gpt_dispatch.h"
#include "gpt_kvar.h"

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

// Step 3: this wave's share of V = W B, folded into ssq = sum of squares and crs = sum of products with the k* column of the
// lane's column (lane & 15), over the rows the lane holds.  Wf: tile (ib, kb) at ib (ib + 1) / 2 + kb, inside it
// [k4][g][q][lane][p] (k_pack_w); the image: row n, column c at 16 n + c, so that k4-step k is the 64 consecutive doubles at 64 k.
__device__ __forceinline__ void stab_sweep(const double* __restrict__ Wf, const int N, const double* __restrict__ img, const int w,
                                           const int lane, double& ssq, double& crs) {
    typedef El<double>::AF AF;
    constexpr int PF = 4;                             // A fragments in flight (k4-steps ahead); divides 16
    const d2* const wf2 = reinterpret_cast<const d2*>(Wf);
    const int ngroups = (N + 63) >> 6;
    ssq = 0.0; crs = 0.0;
    for (int G = w; G < ngroups; G += (G & 7) < 4 ? 7 - 2 * (G & 7) : 1 + 2 * (7 - (G & 7))) {
        // (wave w: groups w, 7 - w, 8 + w, 15 - w)
        const int ib = G >> 3, g = G & 7;
        const int left = N - 64 * G;                  // rows of the model in this group
        const int rmax = left >= 64 ? 4 : (left + 15) >> 4;      // row tiles with a row below N
        const int ksteps = 16 * (G + 1), kdiag = 16 * G;      // the group's own 64 x 64 block of W starts at k4-step kdiag
        auto aptr = [&](const int k4) {
            return wf2 + ((size_t)(ib * (ib + 1) / 2 + (k4 >> 7)) * (WT_TILE_DOUBLES / 2) + (size_t)(((k4 & (WT_K4 - 1)) * WT_GROUPS + g) * El<double>::A_GROUP));
        };
        AF a[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) El<double>::lda(a[i], aptr(i), lane);
        d4 acc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = d4{0.0, 0.0, 0.0, 0.0};
        for (int k4 = 0; k4 < ksteps; k4 += PF) {
            // row tile r of the group is zero from k4-step kdiag + 4 (r + 1) on: it runs to its diagonal only
            const int r0 = k4 >= kdiag ? (k4 - kdiag) >> 2 : 0;
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const double b = img[(size_t)(k4 + i) * 64 + lane];
                const AF cur = a[i];
                const int kn = k4 + i + PF < ksteps ? k4 + i + PF : ksteps - 1;      // clamped: redundant, in bounds
                El<double>::lda(a[i], aptr(kn), lane);
                if (r0 <= 0 && rmax > 0) acc[0] = El<double>::mfma(cur.lo[0], b, acc[0]);
                if (r0 <= 1 && rmax > 1) acc[1] = El<double>::mfma(cur.lo[1], b, acc[1]);
                if (r0 <= 2 && rmax > 2) acc[2] = El<double>::mfma(cur.hi[0], b, acc[2]);
                if (rmax > 3) acc[3] = El<double>::mfma(cur.hi[1], b, acc[3]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double v = acc[r][e];
                ssq += v * v;
                crs += v * __shfl(v, lane & ~3);
            }
    }
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
    bool alive = m < a.M;
    if (alive && t_begin > 0 && __builtin_amdgcn_readfirstlane(a.steps_done[m]) != t_begin) alive = false;     // ended in an earlier launch
    const bool entered = alive;
    auto path_row = [&](const int64_t t) { return a.path + (m * ((int64_t)T + 1) + t) * D; };
    auto step_row = [&](double* const p, const int64_t t) { return p + (m * (int64_t)T + t) * D; };
    double y[D], guess[D];
    bool have_guess = true;
#pragma unroll
    for (int d = 0; d < D; ++d) { y[d] = 0.0; guess[d] = 0.0; }
    if (alive) {
        if (t_begin == 0) {
            have_guess = a.X0 != nullptr;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                y[d] = a.Y0[m * D + d];
                guess[d] = a.X0 ? a.X0[m * D + d] : 0.0;
                if (lane == 0) path_row(0)[d] = y[d];
            }
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                y[d] = path_row(t_begin)[d];
                guess[d] = a.state[m * D + d];
            }
        }
    }
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
                for (int d = 0; d < D; ++d) x[d] = y[d];
            } else {
                status = chain_invert<D>(a.st, a.K, a.rtol, a.max_passes, Tt, lane, have_guess, guess, y, x, Q, A,
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
        auto total = [&](const int which, const int c) { return ((red[0][which][c] + red[1][which][c]) + red[2][which][c]) + red[3][which][c]; };
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
            yn[d] = euler_step(y[d], a.dt, vel[d]);
            ok = ok && __builtin_isfinite(yn[d]);
        }
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (a.vel) step_row(a.vel, t)[d] = vel[d];
                if (a.x) step_row(a.x, t)[d] = x[d];
                if (s.f) step_row(s.f, t)[d] = f[d];
                if (s.dvar) step_row(s.dvar, t)[d] = g[d];
            }
            if (s.var) s.var[m * (int64_t)T + t] = var;
        }
        if (__builtin_amdgcn_readfirstlane(ok ? 1 : 0)) {      // (every lane holds the same value)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (lane == 0) path_row((int64_t)t + 1)[d] = yn[d];
                y[d] = yn[d];
                guess[d] = x[d];
            }
            have_guess = true;
        } else {                                      // ended at step t: nothing after it exists
            alive = false;
            t_stop = t;
            if (lane == 0) live[w] = 0;
            const double nan = __builtin_nan("");
            for (int64_t i = ((int64_t)t + 1) * D + lane; i < ((int64_t)T + 1) * D; i += 64) path_row(0)[i] = nan;
            for (int64_t i = ((int64_t)t + 1) * D + lane; i < (int64_t)T * D; i += 64) {
                if (a.vel) step_row(a.vel, 0)[i] = nan;
                if (a.x) step_row(a.x, 0)[i] = nan;
                if (s.f) step_row(s.f, 0)[i] = nan;
                if (s.dvar) step_row(s.dvar, 0)[i] = nan;
            }
            if (s.var)
                for (int64_t i = (int64_t)t + 1 + lane; i < T; i += 64) s.var[m * (int64_t)T + i] = nan;
        }
    }
    if (!entered || lane != 0) return;
    a.steps_done[m] = t_stop;
    a.status[m] = status;
    if (t_stop == t_end && alive && t_end < T) {
#pragma unroll
        for (int d = 0; d < D; ++d) a.state[m * D + d] = guess[d];
    }
}

void launch_rollout_stab(hipStream_t st, int D, const RolloutStabArgs& a) {
    if (a.r.M <= 0) return;
    const dim3 grid((unsigned)((a.r.M + 3) / 4));         // four trajectories per workgroup (M < 2^31: the grid fits)
    // (the image of the largest admitted model, whatever NP is: launch_lds opts a kernel into one size, once per device)
    constexpr size_t lds = (size_t)ROLLOUT_STAB_MAX_N * 16 * sizeof(double);
    with_small_dim(D, [&](auto d) { launch_lds<k_rollout_stab<decltype(d)::value>>(grid, dim3(256), lds, st, a); });
}

}  // namespace gpt
