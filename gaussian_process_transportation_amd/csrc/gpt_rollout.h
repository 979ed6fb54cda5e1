// The transported policy integrated along whole paths (gpt_rollout.hip, gpt_rollout_host.hip): M trajectories, T explicit Euler
// steps y_{t+1} = y_t + dt v(y_t), v the mean policy of gpt_chain.h pulled back through K maps, 0 <= K <= CHAIN_MAX (K = 0: the
// dynamics rolls out itself, v = its mean)  (internal header; plain C++, it also compiles under g++ for the sanitizer builds).
// Every pointer is device memory, fp64 unless it says int; the arrays of a trajectory are contiguous (trajectory-major).  A
// trajectory ends at the first step whose inverse is not CONVERGED or whose y_{t+1} is not finite: that step's x and vel are
// still recorded, no y_{t+1} is, and every later row is NaN.  (The device code of these rules, for the three rollout kernels:
// gpt_rollout_body.h.)
#pragma once
#include "gpt_chain.h"

#include <climits>
#include <cstdlib>

namespace gpt {

// Steps a launch advances a trajectory by, at most (the environment's GPT_ROLLOUT_STEPS_PER_LAUNCH overrides).  Measured with two maps
// of 8192 points, D = 3, M = 1024 (profiles/rollout_policy.txt): 64 steps are 13 ms, 128 steps 50 ms, 256 steps 132 ms; a launch
// is to stay well below 50 ms on a card that others share.
constexpr int ROLLOUT_STEPS_PER_LAUNCH = 64;

// steps a launch advances a trajectory by: a long rollout is many short kernels, never one long-running one (read per call)
inline int rollout_steps_per_launch(const int by_default) {
    if (const char* e = std::getenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= INT_MAX) return (int)v;
    }
    return by_default;
}

struct RolloutArgs {
    int64_t M;
    int K;                               // 0 .. CHAIN_MAX
    ChainStage st[CHAIN_MAX];
    ChainModel dyn;
    const double* Y0;                    // (M,D) starts
    const double* X0;                    // (M,D) guesses of the source-space preimages of the starts, or null
    double rtol;                         // as ChainArgs
    int max_passes;
    double dt;
    int T;                               // steps of the whole call
    int t_begin, t_end;                  // this launch evaluates steps t_begin .. t_end - 1 of the trajectories still alive
    double* path;                        // (M,T+1,D) row 0 = Y0 (written by the launch with t_begin == 0)
    double* vel;                         // (M,T,D) or null
    double* x;                           // (M,T,D) or null
    int* steps_done;                     // (M) steps whose y_{t+1} was recorded; == t_end after a launch: alive
    int* status;                         // (M) INV_* of the last step evaluated
    double* state;                       // (M,D) x of step t_end - 1, the guess of step t_end: carried to the next launch
};

#ifdef __HIPCC__
// y + (dt v), the product and the sum rounded separately.  (The compiler contracts a product and a sum into one fused multiply-add
// wherever it may, the _rn intrinsics included: they are plain operators.  The pragma is what forbids it here.)  The step of
// k_rollout (gpt_rollout.hip), k_rollout_stab (gpt_rollout_stab.hip) and k_rollout_sampled (gpt_rollout_sampled.hip).
__device__ __forceinline__ double euler_step(const double y, const double dt, const double v) {
#pragma clang fp contract(off)
    const double p = dt * v;
    return y + p;
}
#endif

// one wave per trajectory; trajectories that ended in an earlier launch return at once
void launch_rollout(hipStream_t s, int D, const RolloutArgs& a);

// arrays of gpt_rollout_policy, in the order of its arguments; ints: steps_done, status
enum { RO_Y0 = 0, RO_X0, RO_PATH, RO_VEL, RO_X, RO_STEPS, RO_STATUS, RO_COUNT };
constexpr int RO_INPUTS = 2;             // RO_Y0, RO_X0 travel to the device, the rest from it
constexpr int64_t ROLLOUT_CHUNK_ROWS = 1 << 17;   // path rows per chunk of the host call: max(1, ROLLOUT_CHUNK_ROWS / (T + 1)) trajectories

}  // namespace gpt
