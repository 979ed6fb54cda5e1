// Paths of functions drawn from the dynamics posterior for gfx950 (MI355X): the step of gpt_rollout_sampled.h inside the loop of
// k_rollout.  The reference draws the transported demonstration (sample_transportation, GaussianProcess.samples); what follows the
// policy when the dynamics is one such function, it does not draw.
//
//  k_rollout_sampled : one workgroup of four waves owns sixteen paths, the columns of one MFMA tile; wave w owns columns 4w .. 4w+3.
//               What is the same in every lane of a path's wave (y, the guess, x, f, the push-forward's matrices, the flags) lives
//               in LDS between the phases, one record per path, written by lane 0.  A step:
//                 1. body      each wave, its four paths in turn: x_t = Phi^-1(y_t) (chain_invert; K = 0: x_t = y_t), f_t = mean(x_t)
//                 2. image     each wave writes the k* columns of its four paths for every source into a rows x 16 image in LDS
//                              (rows >= N, the columns of an ended path and of a path past P: zero): one lane per source row, the
//                              distances and the kernel value of stab_columns, the k* column only, so any of the four kernels
//                 3. sweep     after a barrier the four waves sweep Wf with v_mfma_f64_16x16x4_f64 (rollout_w_sweep of
//                              gpt_rollout_body.h); the finished C tiles are u_t = W k*(x_t) of the sixteen paths and go to U[t]
//                              in global memory, 64 consecutive doubles per store (row n, column c at 16 n + c: the C tile)
//                 4. cross     after a barrier the waves share s = 0 .. t in blocks of four: u_t . u_s for sixteen paths at once,
//                              lane (c, q) sums rows q, q + 4, .. < N ascending, two shuffles add the four q; sixteen results
//                              per s go to cb[s]
//                 5. finish    after a barrier each wave, its four live paths in turn: lane l owns the elements l, l + 64, l + 128,
//                              l + 192 of the new factor row: c_ts = k(x_t, x_s) - cb[s], then the substitution column by column,
//                              s ascending: the pivot g_ts = c_ts / g_ss is a broadcast, every lane with s < r < t subtracts
//                              g_ts g_rs, reading column s of the factor (stored transposed, so that a column is consecutive);
//                              the squares and the draw are summed as the pivots come, in the order of gpt_rollout_sampled.h.
//                              Then the degenerate rule, the push-forward (chain_push), the Euler step, the step's rows, the end
//                              rule of k_rollout (entering a launch, the NaN rows after an end, leaving: gpt_rollout_body.h).
//               MFMA columns do not mix and every order is fixed by N, t and the lane layout alone: a path's values do not depend
//               on P, on its neighbours, alive or ended, on its column, nor on the launch cuts (everything a later launch needs is
//               in global memory; it resumes from steps_done).  Whether any path is alive is read after the barrier of step 2 from
//               flags set in step 5 of the step before, so a workgroup leaves together, one (empty) image late.
#include "gpt_rollout_sampled.h"
#include "gpt_rollout_body.h"
#include "gpt_chain_body.h"
#include "gpt_dispatch.h"

namespace gpt {

// what every lane of a path's wave agrees on, between the phases of a step and between steps
struct SampledPath {
    double y[3], guess[3], x[3], f[3], Q[9], A[9];
    int alive, entered, have_guess, status, t_stop;
};

// c k(a, b) of the dynamics for two points given as q = a / (sqrt2 l) and b: the arithmetic of a source row against a point
// (inv_diffs), the row being b / l
template <int KT, int D>
__device__ __forceinline__ double sampled_prior(const ChainModel& m, const double* __restrict__ Tt, const double (&q)[D], const double* __restrict__ b) {
    d4 xs{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int d = 0; d < D; ++d) xs[d] = b[d] * m.inv_ls[d];
    double df[D];
    const double hh = inv_diffs<D>(xs, q, df);
    return kernel_tab<KT>(hh, m.lnc, Tt);
}

// Step 2: the four k* columns of this wave, `col` = image + 4 w; x of path j of the wave at ps[j].x, live or not at ps[j].alive
template <int KT, int D>
__device__ __forceinline__ void sampled_columns(const ChainModel& m, const int rows, const double* __restrict__ Tt, const int lane,
                                                const SampledPath* __restrict__ ps, double* __restrict__ col) {
    double q[4][D];
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        live[j] = ps[j].alive != 0;
#pragma unroll
        for (int d = 0; d < D; ++d) q[j][d] = ps[j].x[d] * (m.inv_ls[d] * 0.70710678118654752440);
    }
    for (int n = lane; n < rows; n += 64) {
        d4 b{0.0, 0.0, 0.0, 0.0};
        if (n < m.N) {
            const d4 xs = *reinterpret_cast<const d4*>(m.Xs + (size_t)n * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double df[D];
                const double hh = inv_diffs<D>(xs, q[j], df);
                const double kv = kernel_tab<KT>(hh, m.lnc, Tt);
                b[j] = live[j] ? kv : 0.0;
            }
        }
        *reinterpret_cast<d4*>(col + (size_t)n * 16) = b;
    }
}

// Step 3: this wave's share of u = W B (rollout_w_sweep), stored to `u` (row n, column c at 16 n + c): element e of row tile r of
// group G is the 64 doubles at 16 (64 G + 16 r + 4 e).  Row tiles with no row below N are stored as zeros.
__device__ __forceinline__ void sampled_sweep(const double* __restrict__ Wf, const int N, const double* __restrict__ img, const int w,
                                              const int lane, double* __restrict__ u) {
    rollout_w_sweep(Wf, N, img, w, lane, [&](const int G, const d4 (&acc)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) u[(size_t)(64 * G + 16 * r + 4 * e) * 16 + lane] = acc[r][e];
    });
}

// Step 4: u_t . u_s for s = 0 .. t, sixteen paths at once; wave w takes the blocks of four s numbered w, w + 4, ..
__device__ __forceinline__ void sampled_cross(const double* __restrict__ U, const size_t ustep, const int N, const int t, const int w,
                                              const int lane, double* __restrict__ cb) {
    const double* const ut = U + (size_t)t * ustep;
    for (int s0 = 4 * w; s0 <= t; s0 += 16) {
        const double* us[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) us[e] = U + (size_t)(s0 + e <= t ? s0 + e : t) * ustep;      // (clamped: in bounds, not stored)
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
        for (int n = lane >> 4; n < N; n += 4) {      // (eight rows of loads in flight: the loop runs at their latency)
            const size_t at = (size_t)n * 16 + (lane & 15);
            const double a = ut[at];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fma(a, us[e][at], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double v = acc[e];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);                    // a + b on one side, b + a on the other: the same bits in all four
            if (lane < 16 && s0 + e <= t) cb[(size_t)(s0 + e) * 16 + lane] = v;
        }
    }
}

// the value of chunk i (wave-uniform) of a lane's four
__device__ __forceinline__ double pick4(const double (&v)[4], const int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }

// Step 5, the factor row of one path: cr[i] = c_tr of r = lane + 64 i on entry, g_tr on return (r < t); dsum = sum_s g_ts^2 and
// acc[d] = sum_s g_ts z_s,d over s < t, s ascending.  gt: the path's transposed factor, column s at gt + s ld.  The columns are
// read four pivots at a time, the next four while these are used: a pivot does not wait for memory.
template <int D>
__device__ __forceinline__ void sampled_row(const double* __restrict__ gt, const int ld, const int t, const int lane, double (&cr)[4],
                                            const double (&dg)[4], const double (&z)[4][D], double& dsum, double (&acc)[D]) {
    constexpr int B = 4;
    dsum = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.0;
    auto columns = [&](const int s0, double (&col)[B][4]) {
#pragma unroll
        for (int e = 0; e < B; ++e)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = lane + 64 * i;
                col[e][i] = (r > s0 + e && r < t) ? gt[(size_t)(s0 + e) * ld + r] : 0.0;      // (s0 + e >= t: no lane reads)
            }
    };
    double col[B][4], nxt[B][4];
    columns(0, col);
    for (int s0 = 0; s0 < t; s0 += B) {
        columns(s0 + B, nxt);
#pragma unroll
        for (int e = 0; e < B; ++e) {
            const int s = s0 + e;
            if (s < t) {                               // (wave-uniform)
                const int i = s >> 6, sl = s & 63;
                const double g = __shfl(pick4(cr, i), sl) / __shfl(pick4(dg, i), sl);
                dsum = sampled_draw(dsum, g, g);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double zi[4] = {z[0][d], z[1][d], z[2][d], z[3][d]};
                    acc[d] = sampled_draw(acc[d], g, __shfl(pick4(zi, i), sl));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = lane + 64 * k;
                    if (r == s) cr[k] = g;
                    else if (r > s && r < t) cr[k] -= g * col[e][k];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < B; ++e)
#pragma unroll
            for (int k = 0; k < 4; ++k) col[e][k] = nxt[e][k];
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_rollout_sampled(RolloutSampledArgs s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char img_raw[];      // the k* image: rows x 16 doubles
    double* const img = reinterpret_cast<double*>(img_raw);
    __shared__ double Tt[256];
    __shared__ SampledPath ps[ROLLOUT_SAMPLED_TILE];
    const RolloutArgs& a = s.r;
    Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t m0 = (int64_t)blockIdx.x * ROLLOUT_SAMPLED_TILE;
    const int T = a.T, t_begin = a.t_begin, t_end = a.t_end, N = a.dyn.N;
    const int rows = sampled_u_rows(N), ld = sampled_ld(T);
    const size_t ustep = (size_t)rows * 16;
    double* const U = s.U + (size_t)blockIdx.x * T * ustep;
    double* const cb = s.cb + (size_t)blockIdx.x * ((size_t)T + 1) * 16;
    const double cn = s.c + s.nugget;
    const double nan = __builtin_nan("");

#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * w + j;
        const int64_t m = m0 + c;
        const bool alive = rollout_enters(a, m);
        if (lane == 0) {
            SampledPath& P = ps[c];
            P.alive = P.entered = alive ? 1 : 0;
            P.have_guess = 1; P.status = INV_CONVERGED; P.t_stop = t_end;
#pragma unroll
            for (int d = 0; d < 3; ++d) { P.y[d] = 0.0; P.guess[d] = 0.0; P.x[d] = 0.0; P.f[d] = 0.0; }
            if (alive) {
                const RolloutCarry<D> e = rollout_entry<D>(a, m, true);
                P.have_guess = e.have_guess;
#pragma unroll
                for (int d = 0; d < D; ++d) { P.y[d] = e.y[d]; P.guess[d] = e.guess[d]; }
            }
        }
    }
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
        // ---- 1. body
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            SampledPath& P = ps[4 * w + j];
            if (!P.alive) continue;
            double y[D], guess[D], x[D], f[D], Q[D][D], A[D][D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                y[i] = P.y[i]; guess[i] = P.guess[i]; x[i] = 0.0; f[i] = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) { Q[i][d] = 0.0; A[i][d] = 0.0; }
            }
            int status = INV_CONVERGED;
            if (a.K == 0) {
#pragma unroll
                for (int d = 0; d < D; ++d) x[d] = y[d];
            } else {
                status = chain_invert<D>(a.st, a.K, a.rtol, a.max_passes, Tt, lane, P.have_guess != 0, guess, y, x, Q, A,
                                         [](int, const double (&)[D], const double (&)[D], const double (&)[D][D], int, int, double) {});
            }
            ch_mean<D>(a.dyn, Tt, lane, x, f);
            if (lane == 0) {
                P.status = status;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    P.x[i] = x[i]; P.f[i] = f[i];
#pragma unroll
                    for (int d = 0; d < D; ++d) { P.Q[i * 3 + d] = Q[i][d]; P.A[i * 3 + d] = A[i][d]; }
                }
            }
        }
        __syncthreads();                              // (the records: lane 0 wrote, every lane reads)
        // ---- 2. image
        switch (a.dyn.ktype) {
            case KT_MATERN12: sampled_columns<KT_MATERN12, D>(a.dyn, rows, Tt, lane, ps + 4 * w, img + 4 * w); break;
            case KT_MATERN32: sampled_columns<KT_MATERN32, D>(a.dyn, rows, Tt, lane, ps + 4 * w, img + 4 * w); break;
            case KT_MATERN52: sampled_columns<KT_MATERN52, D>(a.dyn, rows, Tt, lane, ps + 4 * w, img + 4 * w); break;
            default: sampled_columns<KT_RBF, D>(a.dyn, rows, Tt, lane, ps + 4 * w, img + 4 * w);
        }
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int c = 0; c < ROLLOUT_SAMPLED_TILE; ++c) any |= ps[c].alive;
        if (!any) break;                              // (the same for all four waves: set before the barrier above)
        // ---- 3. sweep
        sampled_sweep(s.Wf, N, img, w, lane, U + (size_t)t * ustep);
        __threadfence_block();
        __syncthreads();
        // ---- 4. cross products
        sampled_cross(U, ustep, N, t, w, lane, cb);
        __threadfence_block();
        __syncthreads();
        // ---- 5. finish
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * w + j;
            SampledPath& P = ps[c];
            if (!P.alive) continue;
            const int64_t m = m0 + c;
            double y[D], x[D], f[D], Q[D][D], A[D][D], q[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                y[i] = P.y[i]; x[i] = P.x[i]; f[i] = P.f[i];
                q[i] = x[i] * (a.dyn.inv_ls[i] * 0.70710678118654752440);
#pragma unroll
                for (int d = 0; d < D; ++d) { Q[i][d] = P.Q[i * 3 + d]; A[i][d] = P.A[i * 3 + d]; }
            }
            int status = P.status;
            if (lane == 0) {                          // x_t joins the path's points (earlier rows are read below: other lanes, other rows)
#pragma unroll
                for (int d = 0; d < D; ++d) step_row<D>(a, a.x, m, t)[d] = x[d];
            }
            double* const gt = s.Gt + (size_t)m * T * ld;
            const double* const zp = s.normals + (size_t)m * T * D;
            double cr[4], dg[4], z[4][D];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = lane + 64 * i;
                cr[i] = 0.0; dg[i] = 1.0;
#pragma unroll
                for (int d = 0; d < D; ++d) z[i][d] = 0.0;
                if (r < t) {
                    const double* const xr = step_row<D>(a, a.x, m, r);
                    double kv;
                    switch (a.dyn.ktype) {
                        case KT_MATERN12: kv = sampled_prior<KT_MATERN12, D>(a.dyn, Tt, q, xr); break;
                        case KT_MATERN32: kv = sampled_prior<KT_MATERN32, D>(a.dyn, Tt, q, xr); break;
                        case KT_MATERN52: kv = sampled_prior<KT_MATERN52, D>(a.dyn, Tt, q, xr); break;
                        default: kv = sampled_prior<KT_RBF, D>(a.dyn, Tt, q, xr);
                    }
                    cr[i] = kv - cb[(size_t)r * 16 + c];
                    dg[i] = gt[(size_t)r * ld + r];
#pragma unroll
                    for (int d = 0; d < D; ++d) z[i][d] = zp[(size_t)r * D + d];
                }
            }
            const double pvar = cn - cb[(size_t)t * 16 + c];
            double dsum, acc[D];
            sampled_row<D>(gt, ld, t, lane, cr, dg, z, dsum, acc);
            const double cvar = pvar - dsum;
            const bool degenerate = __builtin_amdgcn_readfirstlane(sampled_degenerate(cvar, cn) ? 1 : 0) != 0;
            const double gtt = degenerate ? nan : sqrt(cvar);
            double fs[D], vel[D], yn[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                acc[d] = sampled_draw(acc[d], gtt, zp[(size_t)t * D + d]);
                fs[d] = f[d] + acc[d];
            }
            if (a.K == 0) {
#pragma unroll
                for (int d = 0; d < D; ++d) vel[d] = fs[d];
            } else {
                chain_push<D>(a.st, a.K, Q, A, fs, vel);
            }
            bool ok = status == INV_CONVERGED && !degenerate;
            if (status == INV_CONVERGED && degenerate) status = ROLLOUT_DEGENERATE;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (degenerate) vel[d] = nan;
                yn[d] = euler_step(y[d], a.dt, vel[d]);
                ok = ok && __builtin_isfinite(yn[d]);
            }
            // the row of the factor: column-wise into the transposed factor, row-wise into chol (a degenerate row: NaN)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = lane + 64 * i;
                const double v = r < t ? cr[i] : (r == t ? gtt : 0.0);
                if (r <= t) gt[(size_t)r * ld + t] = v;
                if (s.chol && r < T) s.chol[((size_t)m * T + t) * T + r] = degenerate ? nan : v;
            }
            if (lane == 0) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if (a.vel) step_row<D>(a, a.vel, m, t)[d] = vel[d];
                    if (s.f) step_row<D>(a, s.f, m, t)[d] = f[d];
                }
                if (s.pvar) s.pvar[m * (int64_t)T + t] = pvar;
                if (s.cvar) s.cvar[m * (int64_t)T + t] = cvar;
            }
            if (__builtin_amdgcn_readfirstlane(ok ? 1 : 0)) {      // (every lane holds the same value)
                if (lane == 0) {
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        path_row<D>(a, m, (int64_t)t + 1)[d] = yn[d];
                        P.y[d] = yn[d];
                        P.guess[d] = x[d];
                    }
                    P.have_guess = 1;
                    P.status = status;
                }
            } else {                                  // ended at step t: nothing after it exists
                if (lane == 0) { P.alive = 0; P.t_stop = t; P.status = status; }
                rollout_end_fill<D>(a, RolloutOwn{{s.f, nullptr}, {s.pvar, s.cvar}, s.chol}, m, t, lane);
            }
        }
        __syncthreads();                              // (the records again, and the flags the next step's exit reads)
    }
    if (lane != 0) return;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * w + j;
        const SampledPath& P = ps[c];
        if (!P.entered) continue;
        rollout_leave<D>(a, m0 + c, P.t_stop, P.status, P.alive != 0, P.guess);
    }
}

void launch_rollout_sampled(hipStream_t st, int D, const RolloutSampledArgs& a) {
    if (a.r.M <= 0) return;
    const dim3 grid((unsigned)((a.r.M + ROLLOUT_SAMPLED_TILE - 1) / ROLLOUT_SAMPLED_TILE));
    // (the image of the largest admitted model, whatever N is: launch_lds opts a kernel into one size, once per device)
    constexpr size_t lds = (size_t)ROLLOUT_STAB_MAX_N * 16 * sizeof(double);
    with_small_dim(D, [&](auto d) { launch_lds<k_rollout_sampled<decltype(d)::value>>(grid, dim3(256), lds, st, a); });
}

}  // namespace gpt
