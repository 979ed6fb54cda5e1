// Greedy maximum-variance subset selection over a point pool — gpt_select_greedy (include/gpt_hip.h), the device side of
// ActiveLearningGaussianProcess.  With the hyper-parameters held fixed, "insert the pool point of largest posterior
// variance, refit, repeat" is a pivoted Cholesky factorisation of the pool's kernel matrix with the diagonal pivot rule:
// the residual diagonal d is the posterior variance.  One insertion is one new column of the pool factor P (N x mp,
// row-major: a pool point's row is contiguous):
//     P[i, j] = (k(x_i, x_p) - P[i, :j] . P[p, :j]) / sqrt(d[p] + alpha),   d[i] -= P[i, j]^2
// for EVERY pool row i (selected rows included: their d stays sklearn's predictive variance at a training point), and the
// same pass finds each workgroup's (max d, lowest index) over the rows still alive.  A second one-workgroup launch reduces
// the partials in a fixed order to the next pivot, which never leaves the device.  A prescribed pivot (the initial
// subset) runs the same two kernels; the reduction then reads the pivot from the list instead of choosing it.
//
// sel_column is a bandwidth kernel: step j streams 8 N j bytes of P.  A group of LPR lanes (8, 16 or 64: short rows would
// leave most of a wave idle) owns one row at a time and reads it with 16-byte loads against the pivot row's first j
// entries, staged once per workgroup in LDS (the first SEL_LDS_COLS of them; a longer pivot row's tail is read from
// global memory, where every group reads the same addresses).  k is evaluated in scaled coordinates (rows of 4 / 8 / 16
// doubles, gpt_common.h) with the table exp of gpt_exp.h.
//
// Device side only: the kernels and the launcher of gpt_select.h.  The entry point is in gpt_select_host.hip.
#include "gpt_select.h"
#include "gpt_exp.h"

#include <climits>
#include <cmath>

namespace gpt {
namespace {

constexpr int SEL_LDS_COLS = 4096;       // pivot-row entries staged in LDS (32 KB); a multiple of 2 * 64

__device__ __forceinline__ bool sel_better(const double da, const int ia, const double db, const int ib) {
    return da > db || (da == db && ia < ib);
}

__global__ __launch_bounds__(SEL_NT) void sel_scale(const double* __restrict__ X, const double* __restrict__ inv_ls, double* __restrict__ Xs,
                                                    int N, int D, int stride) {
    const int64_t e = (int64_t)blockIdx.x * SEL_NT + threadIdx.x;
    if (e >= (int64_t)N * stride) return;
    const int i = (int)(e / stride), k = (int)(e % stride);
    Xs[e] = k < D ? X[(int64_t)i * D + k] * inv_ls[k] : 0.0;
}

__global__ __launch_bounds__(SEL_NT) void sel_init(SelArgs a) {
    const int64_t i = (int64_t)blockIdx.x * SEL_NT + threadIdx.x;      // N may lie within SEL_NT of 2^31
    if (i < a.N) { a.d[i] = a.base_var; a.alive[i] = 1; }
    if (i == 0) a.pivd[0] = a.base_var;
}

template <int LPR>
__global__ __launch_bounds__(SEL_NT) void sel_column(SelArgs a, int j) {
    __shared__ __attribute__((aligned(16))) double Lrow[SEL_LDS_COLS];
    __shared__ double T[256];
    __shared__ double xp[MAX_D];
    __shared__ double wd[SEL_NT / 64];
    __shared__ int wi[SEL_NT / 64];
    if (*a.fail) return;
    const double piv = a.pivd[j] + a.alpha;
    if (!(piv > 0.0)) {                       // the same value in every workgroup: all of them leave
        if (blockIdx.x == 0 && threadIdx.x == 0) *a.fail = j + 1;
        return;
    }
    const int p = a.selected[j], mp = a.mp, N = a.N, stride = a.stride;
    const double* __restrict__ prow_p = a.P + (size_t)p * mp;
    const int jl = j < SEL_LDS_COLS ? j : SEL_LDS_COLS;
    for (int c = threadIdx.x; c < ((jl + 1) & ~1); c += SEL_NT) Lrow[c] = c < j ? prow_p[c] : 0.0;
    T[threadIdx.x] = g_exp2_table[threadIdx.x];
    if (threadIdx.x < stride) xp[threadIdx.x] = a.Xs[(size_t)p * stride + threadIdx.x];
    __syncthreads();

    const double rs = sqrt(piv);
    constexpr int GROUPS = SEL_NT / LPR;          // rows a workgroup holds at a time
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    double best_d = -INFINITY;
    int best_i = INT_MAX;
    for (int64_t row0 = (int64_t)blockIdx.x * GROUPS; row0 < N; row0 += (int64_t)gridDim.x * GROUPS) {
        const int64_t i = row0 + grp;
        const bool valid = i < N;                  // the shuffles below need whole waves in the loop
        const double* __restrict__ prow = a.P + (size_t)(valid ? i : 0) * mp;
        const int je = valid ? j : 0, jle = valid ? jl : 0;
        d2 acc = {0.0, 0.0};
        int c = 2 * sub;
#pragma unroll 8
        for (; c < jle; c += 2 * LPR) {
            const d2 v = *reinterpret_cast<const d2*>(prow + c);
            const d2 l = *reinterpret_cast<const d2*>(Lrow + c);
            acc.x = fma(v.x, l.x, acc.x);
            acc.y = fma(v.y, l.y, acc.y);
        }
#pragma unroll 4
        for (; c < je; c += 2 * LPR) {            // j > SEL_LDS_COLS: the pivot row's tail from global memory
            const d2 v = *reinterpret_cast<const d2*>(prow + c);
            d2 l = *reinterpret_cast<const d2*>(prow_p + c);
            if (c + 1 >= j) l.y = 0.0;             // column j of row p is being written by its owner
            acc.x = fma(v.x, l.x, acc.x);
            acc.y = fma(v.y, l.y, acc.y);
        }
        double s = acc.x + acc.y;
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (valid) {
            const double* __restrict__ xi = a.Xs + (size_t)i * stride;
            double h = 0.0;
            for (int k = 0; k < stride; k += 2) {
                const d2 x = *reinterpret_cast<const d2*>(xi + k);
                const double u = x.x - xp[k], w = x.y - xp[k + 1];
                h = fma(u, u, h);
                h = fma(w, w, h);
            }
            h *= 0.5;
            double kv;
            switch (a.ktype) {
                case KT_RBF: kv = kernel_tab<KT_RBF>(h, a.lnc, T); break;
                case KT_MATERN12: kv = kernel_tab<KT_MATERN12>(h, a.lnc, T); break;
                case KT_MATERN32: kv = kernel_tab<KT_MATERN32>(h, a.lnc, T); break;
                default: kv = kernel_tab<KT_MATERN52>(h, a.lnc, T); break;
            }
            const double v = (kv - s) / rs;
            const double dn = a.d[i] - v * v;
            const bool mine = (int)i == p;
            if (sub == 0) {
                a.P[(size_t)i * mp + j] = v;
                a.d[i] = dn;
                if (mine) a.alive[i] = 0;
            }
            if (!mine && a.alive[i] && sel_better(dn, (int)i, best_d, best_i)) { best_d = dn; best_i = (int)i; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(best_d, o);
        const int oi = __shfl_xor(best_i, o);
        if (sel_better(od, oi, best_d, best_i)) { best_d = od; best_i = oi; }
    }
    if (threadIdx.x % 64 == 0) { wd[threadIdx.x / 64] = best_d; wi[threadIdx.x / 64] = best_i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SEL_NT / 64; ++w)
            if (sel_better(wd[w], wi[w], best_d, best_i)) { best_d = wd[w]; best_i = wi[w]; }
        a.part_d[blockIdx.x] = best_d;
        a.part_i[blockIdx.x] = best_i;
    }
}

// Pivot of insertion j + 1 after column j: prescribed (the list), or the maximum of the n_part partials — every
// comparison is (larger d, then lower index), so the result does not depend on the order of the reduction.
__global__ __launch_bounds__(SEL_NT) void sel_next(SelArgs a, int j, int n_part) {
    __shared__ double wd[SEL_NT / 64];
    __shared__ int wi[SEL_NT / 64];
    if (*a.fail) return;
    if (j + 1 < a.n_pre) {
        if (threadIdx.x == 0) a.pivd[j + 1] = a.d[a.selected[j + 1]];
        return;
    }
    double best_d = -INFINITY;
    int best_i = INT_MAX;
    for (int t = threadIdx.x; t < n_part; t += SEL_NT)
        if (sel_better(a.part_d[t], a.part_i[t], best_d, best_i)) { best_d = a.part_d[t]; best_i = a.part_i[t]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(best_d, o);
        const int oi = __shfl_xor(best_i, o);
        if (sel_better(od, oi, best_d, best_i)) { best_d = od; best_i = oi; }
    }
    if (threadIdx.x % 64 == 0) { wd[threadIdx.x / 64] = best_d; wi[threadIdx.x / 64] = best_i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SEL_NT / 64; ++w)
            if (sel_better(wd[w], wi[w], best_d, best_i)) { best_d = wd[w]; best_i = wi[w]; }
        a.selected[j + 1] = best_i;          // n_total <= N: a row is still alive whenever a next pivot is asked for
        a.pivd[j + 1] = best_d;
    }
}

// lanes per pool row at insertion j: a row has j doubles, a lane reads two at a time
int sel_lanes(int j) { return j <= 32 ? 8 : (j <= 128 ? 16 : 64); }

}  // namespace

void launch_sel_schedule(hipStream_t s, const SelArgs& a, const double* X, const double* inv_ls, double* Xs, int D, int n_total) {
    const int64_t N = a.N, nxs = N * a.stride;
    hipLaunchKernelGGL(sel_scale, dim3((unsigned)((nxs + SEL_NT - 1) / SEL_NT)), dim3(SEL_NT), 0, s, X, inv_ls, Xs, a.N, D, a.stride);
    hipLaunchKernelGGL(sel_init, dim3((unsigned)((N + SEL_NT - 1) / SEL_NT)), dim3(SEL_NT), 0, s, a);
    for (int j = 0; j < n_total; ++j) {
        const int lpr = sel_lanes(j), groups = SEL_NT / lpr;
        const int64_t want = (N + groups - 1) / groups;
        const int G = (int)(want < SEL_MAX_WG ? want : SEL_MAX_WG);
        if (lpr == 8) hipLaunchKernelGGL(sel_column<8>, dim3(G), dim3(SEL_NT), 0, s, a, j);
        else if (lpr == 16) hipLaunchKernelGGL(sel_column<16>, dim3(G), dim3(SEL_NT), 0, s, a, j);
        else hipLaunchKernelGGL(sel_column<64>, dim3(G), dim3(SEL_NT), 0, s, a, j);
        if (j + 1 < n_total) hipLaunchKernelGGL(sel_next, dim3(1), dim3(SEL_NT), 0, s, a, j, G);
    }
}

}  // namespace gpt
