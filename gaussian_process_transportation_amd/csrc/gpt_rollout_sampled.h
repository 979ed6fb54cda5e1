// Paths of functions drawn from the dynamics posterior (gpt_rollout_sampled.hip, gpt_rollout_sampled_host.hip): the rollout of
// gpt_rollout.h with, in place of the dynamics mean, one function drawn from the posterior of the dynamics GP per path.  The draw
// at step t is conditioned on what the same function was drawn to be at the path's earlier points: a growing Cholesky factor G of
// the path's own posterior covariance, one row per step.  Internal header; plain C++, it also compiles under g++ for the sanitizer
// builds.  Step t of path p, x_t the source-space preimage of y_t under the K maps (K = 0: x_t = y_t), W = L^-1 the inverse factor
// of the dynamics, c its prior variance, z = normals[p] the caller's standard normal numbers (the device generates none):
//   f_t      the dynamics mean at x_t (ch_mean)
//   u_t      = W k*(x_t);  pvar_t = (c + nugget) - u_t . u_t                the marginal posterior variance at x_t
//   c_ts     = k(x_t, x_s) - u_t . u_s   for s < t                         the posterior covariance with the earlier points
//   g_ts     = (c_ts - sum_{r<s} g_tr g_sr) / g_ss, s ascending            a new row of the lower factor G
//   cvar_t   = pvar_t - sum_{s<t} g_ts^2                                   the conditional variance
//   degenerate (sampled_degenerate): the path ends at step t with ROLLOUT_DEGENERATE; else g_tt = sqrt(cvar_t)
//   fs_t,d   = f_t,d + sum_{r<=t} g_tr z_r,d, r ascending (sampled_draw)
//   vel_t    = Q (A_0 (R_jac,0 fs_t)), the push-forward of chain_push (K = 0: vel_t = fs_t)
//   y_{t+1}  = y_t + (dt vel_t), the product and the sum rounded separately
// Only the dynamics is sampled; the maps act through their means.  End rule, NaN filling, steps_done, status of an inverse that
// does not converge, the guesses, negative dt and the cutting into launches: gpt_rollout.h.  A path that ends at step t keeps that
// step's x, f, pvar and cvar (a degenerate end: no vel); every later row is NaN.  With all normals zero the call is the mean
// rollout bit for bit but for the sign of a zero.
#pragma once
#include "gpt_rollout_stab.h"

#include <cmath>

namespace gpt {

// Steps of a sampled rollout, at most: a wave keeps a row of the factor in four registers per lane (64 lanes x 4).
constexpr int ROLLOUT_SAMPLED_MAX_T = 256;
// paths of one workgroup: the columns of one MFMA tile
constexpr int ROLLOUT_SAMPLED_TILE = 16;
// status of a path whose conditional variance fell to the accuracy of the variance itself (after the INV_* values 0 .. 3)
constexpr int ROLLOUT_DEGENERATE = 4;
// A pivot at or below this many ulps of c + nugget is noise: MARGIN x FLOOR_ULPS of tests/posterior_restatement.py, the bound the
// posterior variance is held to.
constexpr double ROLLOUT_SAMPLED_FLOOR_ULPS = 1024.0;
// Device memory the scratch of one chunk of the host call may take (u and the factor; GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES overrides).
constexpr double ROLLOUT_SAMPLED_SCRATCH_BUDGET = 1073741824.0;      // 1 GiB
// Share of the device's free memory the scratch of a _dev call may take (the rule of gpt_select_greedy).
constexpr double ROLLOUT_SAMPLED_MEMORY_SHARE = 0.8;

// Steps a launch advances a path by, at most (GPT_ROLLOUT_STEPS_PER_LAUNCH overrides, as for the mean rollout).  A step's cost grows
// with t (t earlier u to multiply with, t pivots), so the LAST window decides; a launch is to stay below 50 ms (gpt_rollout.h).
// Measured at the largest admitted shape, N_dyn = 1024, D = 3, two maps of 8192 points, T = 256, P = 1024 in launches of 64
// workgroups, every launch from the profiler's kernel trace (profiles/rollout_sampled.txt, tools/rollout_sampled_launches.py),
// first / last launch of a call: 2 steps 3.4 / 15.4 ms, 4 steps 6.7 / 30.7 ms, 8 steps 13.4 / 61.2 ms, 16 steps 27.1 / 122.5 ms.
constexpr int ROLLOUT_SAMPLED_STEPS_PER_LAUNCH = 4;

// the floor of a pivot, and the rule itself: NaN is degenerate
__host__ __device__ inline double sampled_floor(const double cn) { return ROLLOUT_SAMPLED_FLOOR_ULPS * 0x1p-52 * cn; }
__host__ __device__ inline bool sampled_degenerate(const double d, const double cn) { return !(d > sampled_floor(cn)); }

// one term of a running sum, acc + (a b), the product and the sum rounded on their own (no fused multiply-add): the draw
// sum_r g_tr z_r and the squares sum_s g_ts^2, both with the index ascending from acc = 0
__host__ __device__ inline double sampled_draw(const double acc, const double g, const double z) {
#pragma clang fp contract(off)
    const double p = g * z;
    return acc + p;
}

// rows of u a workgroup keeps per step: the 64-row groups of the sweep that hold a row below N
__host__ __device__ inline int sampled_u_rows(const int N) { return ((N + 63) >> 6) << 6; }
// Doubles between two columns of a path's transposed factor: T and a skew of 64 bytes.  With T = 256 itself the columns of a path
// (2 KiB apart) and the paths of a launch (512 KiB apart) would all start on the same memory channels.
__host__ __device__ inline int sampled_ld(const int T) { return T + 8; }
// doubles of scratch a call of P paths takes: u [workgroup][t][row][16], the factor transposed [path][s][sampled_ld(T)], the cross products
// [workgroup][s 0 .. T][16], and x when the caller does not ask for it
inline double sampled_scratch_doubles(const int64_t P, const int64_t T, const int N, const int D, const bool own_x) {
    const double wgs = (double)((P + ROLLOUT_SAMPLED_TILE - 1) / ROLLOUT_SAMPLED_TILE);
    return wgs * (double)T * sampled_u_rows(N) * 16.0 + (double)P * T * sampled_ld((int)T) + wgs * (double)(T + 1) * 16.0 + (own_x ? (double)P * T * D : 0.0);
}

struct RolloutSampledArgs {
    RolloutArgs r;                       // as k_rollout's; r.x is never null here (the caller's array or scratch: the kernel reads it)
    const double* Wf;                    // the dynamics' inverse factor in fragment order (k_pack_w), as RolloutStabArgs
    int NP;                              // its padded size: 512 or 1024
    double c, nugget;
    const double* normals;               // (P,T,D)
    double* f;                           // (P,T,D) or null
    double* pvar;                        // (P,T) or null
    double* cvar;                        // (P,T) or null
    double* chol;                        // (P,T,T) or null: the lower triangle, zeros above it
    double* U;                           // scratch [workgroup][T][sampled_u_rows(N)][16]: u of every step, column = path of the workgroup
    double* Gt;                          // scratch [P][T][sampled_ld(T)]: the factor transposed, Gt[p][s][r] = g_rs for r >= s
    double* cb;                          // scratch [workgroup][T + 1][16]: u_t . u_s of the step in hand, s <= t
};

// one workgroup of four waves owns sixteen paths; paths that ended in an earlier launch only take part in the sweep
void launch_rollout_sampled(hipStream_t s, int D, const RolloutSampledArgs& a);

// arrays of gpt_rollout_sampled, in the order of its arguments; ints: steps_done, status
enum { RP_Y0 = 0, RP_X0, RP_NORMALS, RP_PATH, RP_VEL, RP_X, RP_F, RP_PVAR, RP_CVAR, RP_CHOL, RP_STEPS, RP_STATUS, RP_COUNT };
constexpr int RP_INPUTS = 3;             // RP_Y0, RP_X0, RP_NORMALS travel to the device, the rest from it

}  // namespace gpt
