// Whole paths of the transported policy for gfx950 (MI355X): the reference integrates its policy on the host, 1000 steps of
// pos += vel (plot_traj_evolution); here the loop over the steps runs on the device, around the per-point body of
// k_chain_velocity (gpt_chain_body.h: K Newton inversions, the dynamics mean and the push-forward in one wave).
//
//  k_rollout : one wave owns one trajectory, four waves per workgroup, one barrier at entry for the exp table.  Step t evaluates
//               the body at y_t with the x of step t - 1 as its guess (at t = 0: X0, or none), then y_{t+1} = y_t + (dt vel_t), the
//               product and the sum rounded separately (no fused multiply-add: numpy's y + dt * vel gives the same bits).  Every
//               value is the same in every lane, every branch on it a scalar one; lane 0 stores each step's rows.  The
//               trajectory ends at the first step whose status is not CONVERGED or whose y_{t+1} is not finite.  A launch
//               evaluates steps t_begin .. t_end - 1; how a trajectory enters one, what it leaves behind and the NaN rows after
//               its end are gpt_rollout_body.h's, shared with the other two rollout kernels; a wave whose trajectory does not
//               enter returns at once.  K = 0: x_t = y_t, vel_t = the dynamics mean.  A trajectory's sums run in a fixed order:
//               its values do not depend on M, on the trajectories around it or on the launch boundaries.
#include "gpt_rollout_body.h"
#include "gpt_chain_body.h"

namespace gpt {

template <int D>
__global__ __launch_bounds__(256) void k_rollout(RolloutArgs a) {
    __shared__ double Tt[256];
    Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
    __syncthreads();                                  // the only barrier
    const int lane = threadIdx.x & 63;
    // (the wave's number goes through readfirstlane: m and every address built on it are scalar, which leaves the vector registers to the body)
    const int64_t m = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (!rollout_enters(a, m)) return;
    const int t_begin = a.t_begin, t_end = a.t_end;
    RolloutCarry<D> c = rollout_entry<D>(a, m, lane == 0);
    int t = t_begin, status = INV_CONVERGED;
    for (; t < t_end; ++t) {
        double x[D], f[D], vel[D], yn[D];
        if (a.K == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = c.y[d];
            ch_mean<D>(a.dyn, Tt, lane, x, vel);
        } else {
            status = chain_point<D>(a.st, a.dyn, a.K, a.rtol, a.max_passes, Tt, lane, c.have_guess, c.guess, c.y, x, f, vel,
                                    [](int, const double (&)[D], const double (&)[D], const double (&)[D][D], int, int, double) {});
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
            }
        }
        if (!__builtin_amdgcn_readfirstlane(ok ? 1 : 0)) break;      // (every lane holds the same value)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (lane == 0) path_row<D>(a, m, (int64_t)t + 1)[d] = yn[d];
            c.y[d] = yn[d];
            c.guess[d] = x[d];
        }
        c.have_guess = true;
    }
    if (t < t_end) rollout_end_fill<D>(a, RolloutOwn{}, m, t, lane);
    if (lane == 0) rollout_leave<D>(a, m, t, status, t == t_end, c.guess);
}

void launch_rollout(hipStream_t s, int D, const RolloutArgs& a) {
    if (a.M <= 0) return;
    const dim3 grid((unsigned)((a.M + 3) / 4));           // one wave per trajectory, four per workgroup (M < 2^31: the grid fits)
    with_small_dim(D, [&](auto d) { hipLaunchKernelGGL((k_rollout<decltype(d)::value>), grid, dim3(256), 0, s, a); });
}

}  // namespace gpt
