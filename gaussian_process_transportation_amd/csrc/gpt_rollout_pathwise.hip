// Whole paths of functions drawn from the dynamics posterior by pathwise conditioning, for gfx950 (MI355X); the definitions:
// gpt_rollout_pathwise.h.  The reference draws its samples jointly at fixed points (GaussianProcess.samples); a function that can be
// evaluated anywhere, for any number of steps and from any number of starts, is what a rollout needs.
//
//  k_rollout_pathwise : k_rollout's layout and step loop (one wave per path, four per workgroup, one barrier at entry for the exp
//               table, every value the same in every lane, lane 0 stores).  The body of a step is k_rollout's with the dynamics
//               mean replaced: chain_invert, then ch_mean on the function's own weight image, the feature sum, and chain_push of
//               their sum.  The feature sum strides the frequencies over the lanes as inv_mean strides the sources and ends in
//               the same butterfly; omega and the amplitudes are read from global memory (a wave reads 64 consecutive rows: whole
//               cache lines, shared by every wave on the same function through L2).  Entry, end rule, NaN filling and leave:
//               gpt_rollout_body.h.  A path's sums run in a fixed order: its values do not depend on M, S, the paths around
//               it, the other functions or the launch boundaries.
#include "gpt_rollout_pathwise.h"
#include "gpt_rollout_body.h"
#include "gpt_chain_body.h"

namespace gpt {

// p = sum_j a_j cos(omega_j . x) + b_j sin(omega_j . x), the same in every lane; amp: the function's (J,2,D)
template <int D>
__device__ __forceinline__ void pathwise_features(const int J, const double* __restrict__ omega, const double* __restrict__ amp, const int lane,
                                                  const double (&x)[D], double (&p)[D]) {
    double acc[D];
#pragma unroll
    for (int o = 0; o < D; ++o) acc[o] = 0.0;
    for (int j = lane; j < J; j += 64) {
        const double* const w = omega + (size_t)j * D;
        const double* const ab = amp + (size_t)j * 2 * D;
        double th = w[0] * x[0];
#pragma unroll
        for (int d = 1; d < D; ++d) th = fma(w[d], x[d], th);
        double sn, cs;
        sincos(th, &sn, &cs);
#pragma unroll
        for (int o = 0; o < D; ++o) acc[o] += ab[o] * cs + ab[D + o] * sn;
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
        double v = acc[o];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);         // the same bits in every lane
        p[o] = v;
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_rollout_pathwise(RolloutPathwiseArgs pa) {
    __shared__ double Tt[256];
    Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
    __syncthreads();                                  // the only barrier
    const RolloutArgs& a = pa.r;
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (!rollout_enters(a, m)) return;
    const int fn = __builtin_amdgcn_readfirstlane(pa.func[m]);
    if (fn < 0 || fn >= pa.S) {                       // (the host entry refuses such a call; here nothing is read out of bounds)
        // no function to follow: the path ends before its first step, every row NaN; later launches do not enter (steps_done = 0)
        if (a.t_begin == 0) {
            rollout_end_fill<D>(a, RolloutOwn{{pa.f, nullptr}, {nullptr, nullptr}, nullptr}, m, -1, lane);
            if (lane == 0) { a.steps_done[m] = 0; a.status[m] = ROLLOUT_NO_FUNCTION; }
        }
        return;
    }
    ChainModel fm = a.dyn;
    fm.A4 = pa.V4 + (size_t)fn * pa.image;
    const double* const amp = pa.amp + (size_t)fn * (size_t)pa.J * 2 * D;
    const int t_begin = a.t_begin, t_end = a.t_end;
    RolloutCarry<D> c = rollout_entry<D>(a, m, lane == 0);
    int t = t_begin, status = INV_CONVERGED;
    for (; t < t_end; ++t) {
        double x[D], u[D], p[D], fs[D], vel[D], yn[D], Q[D][D], A[D][D];
        if (a.K == 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = c.y[d];
        } else {
            status = chain_invert<D>(a.st, a.K, a.rtol, a.max_passes, Tt, lane, c.have_guess, c.guess, c.y, x, Q, A,
                                     [](int, const double (&)[D], const double (&)[D], const double (&)[D][D], int, int, double) {});
        }
        ch_mean<D>(fm, Tt, lane, x, u);
        pathwise_features<D>(pa.J, pa.omega, amp, lane, x, p);
#pragma unroll
        for (int d = 0; d < D; ++d) fs[d] = u[d] + p[d];
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
                if (pa.f) step_row<D>(a, pa.f, m, t)[d] = fs[d];
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
    if (t < t_end) rollout_end_fill<D>(a, RolloutOwn{{pa.f, nullptr}, {nullptr, nullptr}, nullptr}, m, t, lane);
    if (lane == 0) rollout_leave<D>(a, m, t, status, t == t_end, c.guess);
}

void launch_rollout_pathwise(hipStream_t s, int D, const RolloutPathwiseArgs& a) {
    if (a.r.M <= 0) return;
    const dim3 grid((unsigned)((a.r.M + 3) / 4));         // one wave per path, four per workgroup (M < 2^31: the grid fits)
    with_small_dim(D, [&](auto d) { hipLaunchKernelGGL((k_rollout_pathwise<decltype(d)::value>), grid, dim3(256), 0, s, a); });
}

}  // namespace gpt
