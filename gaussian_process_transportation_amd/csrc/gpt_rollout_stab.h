// The variance-stabilised policy integrated along whole paths (gpt_rollout_stab.hip, gpt_rollout_stab_host.hip): the rollout of
// gpt_rollout.h with the reference's stabiliser inside the step (plot_traj_evolution: pos += mean - std * grad_var / |grad_var|).
// Internal header; plain C++, it also compiles under g++ for the sanitizer builds.  Step t of a trajectory, x_t the source-space
// preimage of y_t under the K maps (K = 0: x_t = y_t), W = L^-1 the inverse factor of the dynamics:
//   f_t      the dynamics mean at x_t (ch_mean)
//   u        = W k*(x_t);  var_t = max(0, c + noise - sum_i u_i^2);  g_t,d = -2 sum_i u_i (W d_d k*(x_t))_i
//   s_t      = sqrt(var_t) - std_offset
//   ghat_t   = unit_gradient(g_t)
//   fs_t,d   = stabilised(f_t,d, gain, s_t, ghat_t,d)                     the stabilised source-space policy
//   vel_t    = Q (A_0 (R_jac,0 fs_t)), the push-forward of chain_push (K = 0: vel_t = fs_t)
//   y_{t+1}  = y_t + (dt vel_t), the product and the sum rounded separately
// For K >= 1 the target-space path is, to first order in dt, the image of the source-space stabilised path: the variance that is
// descended is the dynamics' own at the preimage, not that of a GP refitted on the moved demonstration.  End rule, NaN filling,
// steps_done, status, the guesses, negative dt and the cutting into launches: gpt_rollout.h.
#pragma once
#include "gpt_rollout.h"

#include <cmath>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace gpt {

// The dynamics of a stabilised rollout has at most this many sources: its B image (NP x 16 doubles, NP the sources padded to a
// multiple of 512) is then at most 128 KiB and stays in LDS for the whole step.
constexpr int ROLLOUT_STAB_MAX_N = 1024;

// Steps a launch advances a trajectory by, at most (GPT_ROLLOUT_STEPS_PER_LAUNCH overrides, as for the mean rollout).  Measured at the
// largest admitted shape, N_dyn = 1024, D = 3, two maps of 8192 points, M = 1024 (profiles/rollout_stabilised.txt): 16 steps are
// 13.3 ms, 32 steps 26.4 ms, 64 steps 51.9 ms; a launch is to stay below 50 ms (gpt_rollout.h).
constexpr int ROLLOUT_STAB_STEPS_PER_LAUNCH = 32;

// ghat = g / |g|, the norm taken after scaling by max_d |g_d| so that a tiny gradient does not underflow to a zero norm; ghat = 0
// where every g_d is exactly 0 (k* has underflowed far from the data: the reference divides 0 by 0 there).  A NaN or infinite
// component makes every ghat_d NaN.  Operation order: h_d = g_d / gmax; n = sqrt((h_0^2 + h_1^2) + h_2^2); ghat_d = h_d / n, each
// operation rounded on its own.
template <int D>
__host__ __device__ inline void unit_gradient(const double (&g)[D], double (&ghat)[D]) {
#pragma clang fp contract(off)
    double gmax = 0.0;
    bool zero = true;
    for (int d = 0; d < D; ++d) {
        gmax = std::fmax(gmax, std::fabs(g[d]));
        zero = zero && g[d] == 0.0;
    }
    if (zero) {
        for (int d = 0; d < D; ++d) ghat[d] = 0.0;
        return;
    }
    double h[D], n2 = 0.0;
    for (int d = 0; d < D; ++d) {
        h[d] = g[d] / gmax;
        const double sq = h[d] * h[d];
        n2 = d == 0 ? sq : n2 + sq;
    }
    const double n = std::sqrt(n2);
    for (int d = 0; d < D; ++d) ghat[d] = h[d] / n;
}

// fs = f - ((gain s) ghat), every product and the difference rounded on their own (no fused multiply-add).  (gain = 0 gives f but
// for the sign of a zero: f = -0.0 with a product of -0.0 gives +0.0.)
__host__ __device__ inline double stabilised(const double f, const double gain, const double s, const double ghat) {
#pragma clang fp contract(off)
    const double p = gain * s;
    const double q = p * ghat;
    return f - q;
}

struct RolloutStabArgs {
    RolloutArgs r;                       // as k_rollout's
    // the dynamics' inverse factor in fragment order (k_pack_w).  launch_pack_w multiplies W by the task's scale and launch_var
    // takes the prior variance of the task to go with it; the dynamics here is a single-task model (the entry points refuse the
    // others), whose scale is 1 and whose prior variance is c
    const double* Wf;
    int NP;                              // its padded size: 512 or 1024
    double c, noise;                     // var = max(0, c + noise - |W k*|^2)
    double gain, std_offset;
    double* f;                           // (M,T,D) or null
    double* var;                         // (M,T) or null
    double* dvar;                        // (M,T,D) or null
};

// one workgroup of four waves owns four trajectories; trajectories that ended in an earlier launch only take part in the sweep
void launch_rollout_stab(hipStream_t s, int D, const RolloutStabArgs& a);

// arrays of gpt_rollout_stabilised, in the order of its arguments; ints: steps_done, status
enum { RS_Y0 = 0, RS_X0, RS_PATH, RS_VEL, RS_X, RS_F, RS_VAR, RS_DVAR, RS_STEPS, RS_STATUS, RS_COUNT };
constexpr int RS_INPUTS = 2;             // RS_Y0, RS_X0 travel to the device, the rest from it

}  // namespace gpt
