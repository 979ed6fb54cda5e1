// What the rollout kernels share (device units only): k_rollout (gpt_rollout.hip), k_rollout_stab (gpt_rollout_stab.hip) and
// k_rollout_sampled (gpt_rollout_sampled.hip).  A trajectory's life across launches, whose rules gpt_rollout.h states, and the
// triangular sweep of the packed inverse factor against a 16-column image in LDS.  Nothing here knows which kernel calls it: a
// family passes its arrays and its values.
#pragma once
#include "gpt_rollout.h"
#include "gpt_kvar.h"

namespace gpt {

// ---- a trajectory across launches: between them it lives in its last path row, `state` (the last x) and steps_done

// row t of trajectory m in path (M,T+1,D), and in an (M,T,D) array p
template <int D>
__device__ __forceinline__ double* path_row(const RolloutArgs& a, const int64_t m, const int64_t t) {
    return a.path + (m * ((int64_t)a.T + 1) + t) * D;
}
template <int D>
__device__ __forceinline__ double* step_row(const RolloutArgs& a, double* const p, const int64_t m, const int64_t t) {
    return p + (m * (int64_t)a.T + t) * D;
}

// whether trajectory m takes part in this launch: it exists and has not ended in an earlier launch (wave-uniform)
__device__ __forceinline__ bool rollout_enters(const RolloutArgs& a, const int64_t m) {
    return m < a.M && (a.t_begin == 0 || __builtin_amdgcn_readfirstlane(a.steps_done[m]) == a.t_begin);
}

// What a trajectory carries from step to step.  rollout_entry: that of a trajectory that enters, Y0 / X0 at t_begin == 0 (`store`:
// this lane records row 0 of path), else the last path row and `state`.  By value: the members stay in registers.
template <int D>
struct RolloutCarry {
    double y[D], guess[D];
    bool have_guess;
};
template <int D>
__device__ __forceinline__ RolloutCarry<D> rollout_entry(const RolloutArgs& a, const int64_t m, const bool store) {
    RolloutCarry<D> c;
    c.have_guess = true;
    if (a.t_begin == 0) {
        c.have_guess = a.X0 != nullptr;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            c.y[d] = a.Y0[m * D + d];
            c.guess[d] = a.X0 ? a.X0[m * D + d] : 0.0;
            if (store) path_row<D>(a, m, 0)[d] = c.y[d];
        }
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            c.y[d] = path_row<D>(a, m, a.t_begin)[d];
            c.guess[d] = a.state[m * D + d];
        }
    }
    return c;
}

// the arrays of a family beside path, vel and x: (M,T,D), (M,T) and (M,T,T), null where it has none or the caller wants none
struct RolloutOwn {
    double* vec[2];
    double* sca[2];
    double* chol;
};

// Trajectory m ended at step t, nothing after it exists: NaN in every later row of path, vel, x and `own` (the whole wave)
template <int D>
__device__ __forceinline__ void rollout_end_fill(const RolloutArgs& a, const RolloutOwn& own, const int64_t m, const int t, const int lane) {
    const double nan = __builtin_nan("");
    const int64_t T = a.T;
    for (int64_t i = ((int64_t)t + 1) * D + lane; i < (T + 1) * D; i += 64) path_row<D>(a, m, 0)[i] = nan;
    for (int64_t i = ((int64_t)t + 1) * D + lane; i < T * D; i += 64) {
        if (a.vel) step_row<D>(a, a.vel, m, 0)[i] = nan;
        if (a.x) step_row<D>(a, a.x, m, 0)[i] = nan;
#pragma unroll
        for (double* const p : own.vec)
            if (p) step_row<D>(a, p, m, 0)[i] = nan;
    }
    for (int64_t i = (int64_t)t + 1 + lane; i < T; i += 64) {
#pragma unroll
        for (double* const p : own.sca)
            if (p) p[m * T + i] = nan;
    }
    if (own.chol)
        for (int64_t i = ((int64_t)t + 1) * T + lane; i < T * T; i += 64) own.chol[m * T * T + i] = nan;
}

// Leaving the launch (one lane): steps_done, status, and `state` when the trajectory is alive and steps remain
template <int D>
__device__ __forceinline__ void rollout_leave(const RolloutArgs& a, const int64_t m, const int t_stop, const int status, const bool alive,
                                              const double* const guess) {
    a.steps_done[m] = t_stop;
    a.status[m] = status;
    if (alive && a.t_end < a.T) {
#pragma unroll
        for (int d = 0; d < D; ++d) a.state[m * D + d] = guess[d];
    }
}

// ---- the sweep: wave w's share of C = W B for a 16-column image B in LDS, sixteen columns being one v_mfma_f64_16x16x4_f64 tile
//
// Wf: tile (ib, kb) at ib (ib + 1) / 2 + kb, inside it [k4][g][q][lane][p] (k_pack_w), so that the A fragments of a 64-row group
// for one k4-step are one 2 KiB record, 16 bytes per lane; the image: row n, column c at 16 n + c, so that k4-step k is the 64
// consecutive doubles at 64 k.  This and gpt_kvar.h are the only places that know the layout of Wf.

// The four C tiles of the 64-row group G: a row tile runs k to its diagonal only; row tiles with no row below N are skipped and
// stay zero.  Lane l of a finished tile holds column l & 15, rows (l >> 4) + 4 e in element e: acc[r][e] is row
// 64 G + 16 r + 4 e + (l >> 4) of the product.
__device__ __forceinline__ void rollout_w_group(const double* __restrict__ Wf, const int N, const double* __restrict__ img, const int G,
                                                const int lane, d4 (&acc)[4]) {
    typedef El<double>::AF AF;
    constexpr int PF = 4;                             // A fragments in flight (k4-steps ahead); divides 16
    const d2* const wf2 = reinterpret_cast<const d2*>(Wf);
    const int ib = G >> 3, g = G & 7;
    const int left = N - 64 * G;                      // rows of the model in this group
    const int rmax = left >= 64 ? 4 : (left + 15) >> 4;      // row tiles with a row below N
    const int ksteps = 16 * (G + 1), kdiag = 16 * G;  // the group's own 64 x 64 block of W starts at k4-step kdiag
    auto aptr = [&](const int k4) {
        return wf2 + ((size_t)(ib * (ib + 1) / 2 + (k4 >> 7)) * (WT_TILE_DOUBLES / 2) + (size_t)(((k4 & (WT_K4 - 1)) * WT_GROUPS + g) * El<double>::A_GROUP));
    };
    AF a[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) El<double>::lda(a[i], aptr(i), lane);
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
}

// A wave takes whole 64-row groups, dealt 0 1 2 3 3 2 1 0 per eight groups (wave w: groups w, 7 - w, 8 + w, 15 - w): the triangle
// gives group G 16 (G + 1) k4-steps, and this deal gives every wave the same number where round-robin would give the last wave
// twice the first's.  tile(G, acc) receives the finished C tiles of each of the wave's groups.
template <class Tile>
__device__ __forceinline__ void rollout_w_sweep(const double* __restrict__ Wf, const int N, const double* __restrict__ img, const int w,
                                                const int lane, Tile&& tile) {
    const int ngroups = (N + 63) >> 6;
    for (int G = w; G < ngroups; G += (G & 7) < 4 ? 7 - 2 * (G & 7) : 1 + 2 * (7 - (G & 7))) {
        d4 acc[4];
        rollout_w_group(Wf, N, img, G, lane, acc);
        tile(G, acc);
    }
}

}  // namespace gpt
