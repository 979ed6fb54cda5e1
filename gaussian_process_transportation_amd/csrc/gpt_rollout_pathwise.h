// Paths of WHOLE functions drawn from the dynamics posterior (gpt_rollout_pathwise.hip, gpt_rollout_pathwise_host.hip): the rollout
// of gpt_rollout.h with, in place of the dynamics mean, one of S deterministic functions the caller has drawn by pathwise
// conditioning (Matheron's rule with random Fourier features for the prior):
//   F_s(x) = sum_n k(x, X_n) V_s[n, :]  +  sum_j ( a_sj cos(omega_j . x) + b_sj sin(omega_j . x) )
// Internal header; plain C++, it also compiles under g++ for the sanitizer builds.  Step t of path p, s = func[p], x_t the
// source-space preimage of y_t under the K maps (K = 0: x_t = y_t):
//   u_t      = ch_mean of the dynamics with V_s in the place of its alpha rows (the [NP][4] image A4 uses, one per function)
//   theta_j  = sum_d omega_jd x_t,d, d ascending;  p_t = sum_j a_sj cos(theta_j) + b_sj sin(theta_j): lane l sums j = l, l + 64, ...,
//              then the xor butterfly 32 .. 1 of inv_mean (gpt_newton.h): the same bits in every lane
//   fs_t     = u_t + p_t
//   vel_t    = Q (A_0 (R_jac,0 fs_t)), the push-forward of chain_push (K = 0: vel_t = fs_t)
//   y_{t+1}  = y_t + (dt vel_t), the product and the sum rounded separately
// The cost of a step is O(N + J): no sweep of the inverse factor, no factor of the path, so neither N nor T has a limit of its
// own.  End rule, NaN filling, steps_done, status, the guesses, negative dt and the cutting into launches: gpt_rollout.h.  With
// J = 0 and V_s = alpha the call is the mean rollout bit for bit but for the sign of a zero (u + 0).
#pragma once
#include "gpt_rollout.h"

namespace gpt {

constexpr int PATHWISE_MAX_FREQ = 8192;  // = GPT_PATHWISE_MAX_FREQ of include/gpt_hip.h
// status of a path of the device entry whose func entry names no function (beside the INV_* values 0 .. 3); = GPT_ROLLOUT_NO_FUNCTION
constexpr int ROLLOUT_NO_FUNCTION = -1;

// Steps a launch advances a path by, at most (GPT_ROLLOUT_STEPS_PER_LAUNCH overrides, as for the mean rollout): the largest power of
// two whose longest launch stays below 50 ms (gpt_rollout.h) at the largest admitted shape, two maps of 8192 points, N_dyn = 8192,
// J = 8192, D = 3, 1024 paths.  Every launch from the profiler's kernel trace (profiles/rollout_pathwise.txt,
// tools/rollout_timing.py --pathwise-launches / --pathwise-report): 8 steps 2.9 ms, 16 steps 5.8 ms, 32 steps 11.0 ms, 64 steps
// 21.1 ms, 128 steps 41.4 ms, 256 steps 76.3 .. 79.7 ms.  A step is k_rollout's with the mean taken on the function's weights and the
// feature sum added.
constexpr int ROLLOUT_PATHWISE_STEPS_PER_LAUNCH = 128;

struct RolloutPathwiseArgs {
    RolloutArgs r;                       // as k_rollout's; r.dyn.A4 is not read (the functions bring their own images)
    const int* func;                     // (M) the function of each path, 0 .. S - 1 (a path whose entry is outside ends before its first step)
    int S, J;
    size_t image;                        // doubles per function of V4: 4 NP of the dynamics
    const double* V4;                    // [S][NP][4] the weights in the layout of A4, zero rows from N on
    const double* omega;                 // (J,D)
    const double* amp;                   // (S,J,2,D) cosine amplitudes, then sine amplitudes
    double* f;                           // (M,T,D) fs, or null
};

// one wave per path, four per workgroup; paths that ended in an earlier launch return at once
void launch_rollout_pathwise(hipStream_t s, int D, const RolloutPathwiseArgs& a);

// arrays of gpt_rollout_pathwise that have one row per path, in the order of its arguments; ints: func, steps_done, status
enum { RW_Y0 = 0, RW_X0, RW_FUNC, RW_PATH, RW_VEL, RW_X, RW_F, RW_STEPS, RW_STATUS, RW_COUNT };
constexpr int RW_INPUTS = 3;             // RW_Y0, RW_X0, RW_FUNC travel to the device, the rest from it

}  // namespace gpt
