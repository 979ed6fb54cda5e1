// Fold scan of a batch of small displacement maps — gpt_batch_fold_scan (include/gpt_hip.h).  A transport is x -> x + psi(x) with
// psi the posterior mean of a small exact GP; it is a diffeomorphism only where det(I + d psi / d x) > 0.  The search for a
// fold-free fit (GaussianProcessTransportationDiffeo.optimize_diffeomorphism) scores B candidate hyper-parameters of one data set
// on M points, and wants five numbers per candidate back, not B M D^2 Jacobian entries.  Three kernels:
//     fs_factor  one workgroup per model and size class (n <= 32: 64 threads, n <= 128: 256): bat_factor_body (gpt_batch_device.h,
//                the one text of the factorisation) on K(X) for alpha = K^-1 Y, then, with the surrogate, on K(X + Y) for
//                beta = K(X + Y)^-1 (-Y) in the same workgroup and the same LDS image.  Only alpha and beta leave it.
//     fs_scan    one 64-lane workgroup per (model, 64 queries), a lane per query, as bat_predict tiles them.  The sources, alpha,
//                the surrogate's inputs and beta sit in LDS (12 KB at n = 128, D = 3) and every lane walks them reading the same
//                entry (a broadcast): psi, J, det, z = x + psi, then psi_inv(z) and err, O(n D) per query and no inverse factor.
//                The tile's minimum (with the lowest index attaining it), its count of det <= 0 and its sum and maximum of err
//                are reduced across the wave by a butterfly and written as the tile's partial.
//     fs_reduce  one 64-lane workgroup per model: lane l folds the partials of tiles l, l + 64, .. in turn, then the same butterfly.
// No atomics: the order of every sum and comparison is fixed by (n, D, M_b) alone, so a query's numbers do not depend on the
// other queries and a model's not on the batch, bit for bit.  A lane past the end of its model's queries repeats the last query
// and enters the reductions as the identity (+infinity, 0).
//
// This is a small problem (B = 100, M = 10^4, n = 20: 2 10^7 kernel evaluations); the point is one call and five numbers per
// candidate, not a rate.  Device side only: the kernels and the two launchers of gpt_fold_scan.h.  The entry point is in
// gpt_fold_scan_host.hip.
#include "gpt_fold_scan.h"
#include "gpt_batch_device.h"
#include "gpt_dispatch.h"
#include "gpt_small.h"
#include "../../include/gpt_hip.h"

#include <climits>

namespace gpt {
namespace {

template <int NMAX>
__global__ __launch_bounds__(BatCfg<NMAX>::NT) void fs_factor(FoldScanArgs a) {
    using Cfg = BatCfg<NMAX>;
    constexpr int NT = Cfg::NT, LD = Cfg::LD;
    extern __shared__ __attribute__((aligned(16))) double bat_lds[];
    double* __restrict__ A = bat_lds;                    // NMAX x LD
    double* __restrict__ buf = A + NMAX * LD;            // n x D: y, then W y, then alpha
    double* __restrict__ dinv = buf + NMAX * BAT_MAX_O;  // 1 / L_ii
    __shared__ double red[BAT_RED][NT / 64];

    const int b = a.list[blockIdx.x];
    const int64_t n0 = a.n_begin[b];
    const int n = (int)(a.n_begin[b + 1] - n0);
    const int D = a.D, tid = threadIdx.x;
    const double c = a.c[b], noise = a.noise[b];
    double il[MAX_DIMS];
#pragma unroll
    for (int d = 0; d < MAX_DIMS; ++d) il[d] = d < D ? 1.0 / a.ls[(int64_t)b * a.n_ls + (a.n_ls == 1 ? 0 : d)] : 0.0;

    BatArgs fa{};                                        // what bat_factor_body reads of bat_factor's arguments
    fa.D = D; fa.O = D; fa.n_ls = a.n_ls; fa.jitter = a.jitter;
    for (int pass = 0; pass < (a.surrogate ? 2 : 1); ++pass) {     // the source matrix, then the surrogate's
        fa.X = pass ? a.Xs : a.X;
        fa.Y = pass ? a.Ys : a.Y;
        fa.alpha = pass ? a.beta : a.alpha;
        int* __restrict__ st = pass ? a.sur_status : a.status;
        double sums[BAT_RED];                            // zeroed by the body
        // the body ends with a barrier (block_sum): the image of the first pass is free when the second starts
        if (!bat_factor_body<NMAX, KT_RBF, false>(fa, b, n0, n, c, noise, il, A, buf, dinv, red, sums)) {
            if (tid == 0) st[b] = GPT_E_NOT_PD;          // every thread is here: nothing else of this pass is written
            return;
        }
        if (tid == 0) st[b] = GPT_OK;
    }
}

// (value, index) pairs: the smaller value wins, the lower index on a tie
__device__ __forceinline__ void min_first(double& v, int& i, const double ov, const int oi) {
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// Across the 64 lanes: every lane receives the same four numbers (the operations are commutative, so both lanes of a pair
// compute the same bits).
__device__ __forceinline__ void wave_fold(double& dmin, int& idx, int& nf, double& es, double& em) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        min_first(dmin, idx, __shfl_xor(dmin, o), __shfl_xor(idx, o));
        nf += __shfl_xor(nf, o);
        es += __shfl_xor(es, o);
        em = fmax(em, __shfl_xor(em, o));
    }
}

template <int NMAX, int D>
__global__ __launch_bounds__(BAT_QT) void fs_scan(FoldScanArgs a, int tile0) {
    __shared__ double Xl[NMAX * D], Al[NMAX * D], Xsl[NMAX * D], Bl[NMAX * D], T[256];   // sources, alpha, surrogate inputs, beta, exp table
    const int t = tile0 + blockIdx.x, b = a.tile_model[t], lane = threadIdx.x;
    if (a.status[b] != GPT_OK) return;                    // a model that is not PD: its outputs stay as they were
    const int64_t n0 = a.n_begin[b], ob = a.o_begin[b], Mb = a.o_begin[b + 1] - ob;
    const int n = (int)(a.n_begin[b + 1] - n0);
    const int q = a.tile_q0[t] + lane;
    const bool valid = q < Mb;
    const int64_t ql = valid ? q : Mb - 1;                // a lane past the end repeats the last query and writes nothing
    const bool sur = a.surrogate && a.sur_status[b] == GPT_OK;
    const double lnc = log(a.c[b]);
    const double* __restrict__ ls = a.ls + (int64_t)b * a.n_ls;

    for (int e = lane; e < n * D; e += BAT_QT) {
        Xl[e] = a.X[n0 * D + e];
        Al[e] = a.alpha[n0 * D + e];
        if (sur) { Xsl[e] = a.Xs[n0 * D + e]; Bl[e] = a.beta[n0 * D + e]; }
    }
    for (int e = lane; e < 256; e += BAT_QT) T[e] = g_exp2_table[e];
    double il[D], x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        il[d] = 1.0 / ls[a.n_ls == 1 ? 0 : d];
        x[d] = a.Xq[((a.shared ? 0 : ob) + ql) * D + d];
    }
    __syncthreads();

    // psi_o = sum_k k*_k alpha_ko,  J[o][d] = sum_k k*_k (X_kd - x_d) / l_d^2 alpha_ko
    double m[D], J[D][D];
#pragma unroll
    for (int o = 0; o < D; ++o) {
        m[o] = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) J[o][d] = 0.0;
    }
    for (int k = 0; k < n; ++k) {
        double u[D], h = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) { u[d] = (Xl[k * D + d] - x[d]) * il[d]; h = fma(u[d], u[d], h); }
        const double kv = kernel_tab<KT_RBF>(0.5 * h, lnc, T);
#pragma unroll
        for (int o = 0; o < D; ++o) m[o] = fma(kv, Al[k * D + o], m[o]);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double w = kv * (u[d] * il[d]);
#pragma unroll
            for (int o = 0; o < D; ++o) J[o][d] = fma(w, Al[k * D + o], J[o][d]);
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) J[d][d] += 1.0;
    const double det = sm_det<D>(J);
    double z[D];
#pragma unroll
    for (int d = 0; d < D; ++d) z[d] = x[d] + m[d];

    double err = 0.0;
    if (sur) {                                            // the same value in every lane of the workgroup
        double mi[D];
#pragma unroll
        for (int o = 0; o < D; ++o) mi[o] = 0.0;
        for (int k = 0; k < n; ++k) {
            double h = 0.0;
#pragma unroll
            for (int d = 0; d < D; ++d) { const double u = (Xsl[k * D + d] - z[d]) * il[d]; h = fma(u, u, h); }
            const double kv = kernel_tab<KT_RBF>(0.5 * h, lnc, T);
#pragma unroll
            for (int o = 0; o < D; ++o) mi[o] = fma(kv, Bl[k * D + o], mi[o]);
        }
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) { const double e = m[d] + mi[d]; s = fma(e, e, s); }
        err = sqrt(s);
    }

    if (valid) {
        const int64_t row = ob + q;
        if (a.det) a.det[row] = det;
        if (a.z) {
#pragma unroll
            for (int d = 0; d < D; ++d) a.z[row * D + d] = z[d];
        }
        if (sur && a.err) a.err[row] = err;
    }

    double dmin = valid ? det : __builtin_huge_val(), es = valid ? err : 0.0, em = es;
    int idx = valid ? q : INT_MAX, nf = valid && det <= 0.0 ? 1 : 0;
    wave_fold(dmin, idx, nf, es, em);
    if (lane == 0) {
        a.part[(int64_t)t * FS_PART_D + 0] = dmin; a.part[(int64_t)t * FS_PART_D + 1] = es; a.part[(int64_t)t * FS_PART_D + 2] = em;
        a.ipart[(int64_t)t * FS_PART_I + 0] = idx; a.ipart[(int64_t)t * FS_PART_I + 1] = nf;
    }
}

__global__ __launch_bounds__(64) void fs_reduce(FoldScanArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (a.status[b] != GPT_OK) return;
    const int64_t Mb = a.o_begin[b + 1] - a.o_begin[b];
    const int t0 = a.tile_first[b], t1 = t0 + (int)((Mb + BAT_QT - 1) / BAT_QT);
    double dmin = __builtin_huge_val(), es = 0.0, em = 0.0;
    int idx = INT_MAX, nf = 0;
    for (int t = t0 + lane; t < t1; t += 64) {
        min_first(dmin, idx, a.part[(int64_t)t * FS_PART_D + 0], a.ipart[(int64_t)t * FS_PART_I + 0]);
        nf += a.ipart[(int64_t)t * FS_PART_I + 1];
        es += a.part[(int64_t)t * FS_PART_D + 1];
        em = fmax(em, a.part[(int64_t)t * FS_PART_D + 2]);
    }
    wave_fold(dmin, idx, nf, es, em);
    if (lane != 0) return;
    a.min_det[b] = dmin;
    a.argmin[b] = t1 > t0 ? idx : -1;
    a.n_fold[b] = nf;
    if (a.surrogate && a.sur_status[b] == GPT_OK) { a.err_sum[b] = es; a.err_max[b] = em; }
}

template <int NMAX>
void launch_factor(int count, hipStream_t s, const FoldScanArgs& a) {
    using Cfg = BatCfg<NMAX>;
    if (count < 1) return;
    if constexpr (NMAX > BAT_SMALL_N) launch_lds<fs_factor<NMAX>>(dim3(count), dim3(Cfg::NT), Cfg::factor_lds, s, a);
    else hipLaunchKernelGGL((fs_factor<NMAX>), dim3(count), dim3(Cfg::NT), Cfg::factor_lds, s, a);
}

}  // namespace

void launch_fs_factor(hipStream_t s, int n_small, int n_large, const FoldScanArgs& a) {
    launch_factor<BAT_SMALL_N>(n_small, s, a);
    FoldScanArgs large = a;
    large.list += n_small;
    launch_factor<BAT_MAX_N>(n_large, s, large);
}

void launch_fs_scan(hipStream_t s, int tiles_small, int tiles_large, int64_t B, const FoldScanArgs& a) {
    with_small_dim(a.D, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        if (tiles_small > 0) hipLaunchKernelGGL((fs_scan<BAT_SMALL_N, D>), dim3(tiles_small), dim3(BAT_QT), 0, s, a, 0);
        if (tiles_large > 0) hipLaunchKernelGGL((fs_scan<BAT_MAX_N, D>), dim3(tiles_large), dim3(BAT_QT), 0, s, a, tiles_small);
    });
    hipLaunchKernelGGL(fs_reduce, dim3((unsigned)B), dim3(64), 0, s, a);
}

}  // namespace gpt
