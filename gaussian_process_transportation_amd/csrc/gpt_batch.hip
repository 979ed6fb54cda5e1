// A batch of independent small exact GPs (n <= 128 points each) — gpt_batch_lml_objective, gpt_batch_fit and
// gpt_batch_predict (include/gpt_hip.h).  The reference's transport problems are tiny and numerous (10 .. 20 source points per
// frame pair, hundreds of pairs); padded to 512 rows and factored by a chain of launches each of them costs what a 400-point
// model costs.  Here ONE workgroup owns one model from the Gram matrix to the gradient, and one launch serves every model of a
// size class (n <= 32: 64 threads and 12.5 KB of LDS, so many models share a CU; n <= 128: 256 threads and the 129-column image).
//
// bat_factor is a prologue (the model's rows and hyper-parameters), bat_factor_body (gpt_batch_device.h) and the write of the
// LML, the gradient and the status.  The body keeps the n x n image A in LDS with an odd row stride (column walks hit distinct banks):
//     lower triangle: K, then its Cholesky factor L in place (right-looking, two barriers per column)
//     upper triangle: W^T, W = L^-1, built row by row (row i of W needs row i of L and the finished rows above it; writing
//                     it transposed leaves L readable, so a step has one barrier); 1 / L_ii in a vector of its own
//     alpha = W^T (W y) for the O right-hand sides; LML = -1/2 y.alpha - O sum log L_ii - O n/2 log 2 pi
//     gradient (objective only): 1/2 sum_ij (alpha alpha^T - O K^-1)_ij dK_ij/dtheta with K^-1_ij = sum_k W_ki W_kj from the
//                     image and dK/dtheta regenerated from the coordinates (global memory: beside the 129 KB image and the
//                     16 KB of alpha the CU's 160 KB have no room for them)
// bat_predict: one 64-lane workgroup per (model, 64 queries), a lane per query.  W (packed), the scaled sources and the lane's
// k* column sit in LDS; every lane walks W's rows reading the same entry (a broadcast), so |W k*|^2, |W dk_d|^2 and
// (W dk_d).(W k*) need no reduction across lanes.
//
// Every sum runs in an order fixed by (n, D, O) alone: a model's results do not depend on the batch around it, a query's not
// on the other queries — bit for bit.  That is why the size class is chosen per model, not per batch.
//
// Device side only: the kernels and the two launchers of gpt_batch.h.  The entry points are in gpt_batch_host.hip.  The size
// classes (BatCfg), block_sum, kernel_libm_g and the one text of the factorisation, bat_factor_body, with bat_lml and bat_grad, are
// in gpt_batch_device.h: bat_optimize (gpt_batch_opt.hip) runs the same function once per objective evaluation.
#include "gpt_batch.h"
#include "gpt_batch_device.h"
#include "gpt_dispatch.h"
#include "gpt_exp.h"
#include "../../include/gpt_hip.h"

namespace gpt {
namespace {

template <int NMAX, int KT, bool OBJ>
__global__ __launch_bounds__(BatCfg<NMAX>::NT) void bat_factor(BatArgs a) {
    using Cfg = BatCfg<NMAX>;
    constexpr int NT = Cfg::NT, LD = Cfg::LD;
    extern __shared__ __attribute__((aligned(16))) double bat_lds[];
    double* __restrict__ A = bat_lds;                    // NMAX x LD
    double* __restrict__ buf = A + NMAX * LD;            // n x O: y, then W y, then alpha
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

    double sums[BAT_RED];                                // zeroed by the body
    if (!bat_factor_body<NMAX, KT, OBJ>(a, b, n0, n, c, noise, il, A, buf, dinv, red, sums)) {
        if (tid == 0) a.status[b] = GPT_E_NOT_PD;        // every thread is here: nothing else of the model is written
        return;
    }
    if (tid == 0) {
        if (a.lml) a.lml[b] = bat_lml(sums, n, a.O);
        if (OBJ) bat_grad(sums, c, noise, a.n_ls, a.grad + (int64_t)b * (2 + a.n_ls));
        a.status[b] = GPT_OK;
    }
}

// DW: the dimensions the derivative sums are unrolled over (3, 8 or MAX_DIMS, as coord_width picks; D <= DW)
template <int NMAX, int KT, bool DER, int DW>
__global__ __launch_bounds__(BAT_QT) void bat_predict(BatPredArgs a, int tile0) {
    using Cfg = BatCfg<NMAX>;
    extern __shared__ __attribute__((aligned(16))) double bat_lds[];
    double* __restrict__ Wl = bat_lds;                    // packed rows of W: row i at i (i + 1) / 2
    double* __restrict__ Ks = Wl + Cfg::W_PACKED;         // k*: [k][lane]
    double* __restrict__ Xl = Ks + NMAX * BAT_QT;         // scaled sources: [k][D]
    double* __restrict__ T = Xl + NMAX * MAX_DIMS;        // exp table
    const int t = tile0 + blockIdx.x, b = a.tile_model[t], lane = threadIdx.x;
    if (a.status[b] != GPT_OK) return;                    // a model that is not PD: its outputs stay as they were
    const int64_t n0 = a.n_begin[b], qb = a.q_begin[b];
    const int n = (int)(a.n_begin[b + 1] - n0), D = a.D, O = a.O;
    const int64_t Mb = a.q_begin[b + 1] - qb, q = (int64_t)a.tile_q0[t] + lane;
    const bool valid = q < Mb;
    const int64_t row = qb + (valid ? q : Mb - 1);        // a lane past the end repeats the last query and writes nothing
    const double c = a.c[b], noise = a.noise[b], lnc = log(c);
    const double* __restrict__ ls = a.ls + (int64_t)b * a.n_ls;
    const double* __restrict__ al = a.alpha + n0 * O;

    const double* __restrict__ Wg = a.Wp + a.w_begin[b];
    for (int e = lane; e < n * (n + 1) / 2; e += BAT_QT) Wl[e] = Wg[e];
    for (int e = lane; e < n * D; e += BAT_QT) Xl[e] = a.X[n0 * D + e] / ls[a.n_ls == 1 ? 0 : e % D];
    for (int e = lane; e < 256; e += BAT_QT) T[e] = g_exp2_table[e];
    double il[DW], xs[DW];
#pragma unroll
    for (int d = 0; d < DW; ++d) {
        il[d] = d < D ? 1.0 / ls[a.n_ls == 1 ? 0 : d] : 0.0;
        xs[d] = d < D ? a.Xq[row * D + d] / ls[a.n_ls == 1 ? 0 : d] : 0.0;
    }
    __syncthreads();

    for (int k = 0; k < n; ++k) {
        double h = 0.0;
#pragma unroll
        for (int d = 0; d < DW; ++d)
            if (d < D) { const double u = Xl[k * D + d] - xs[d]; h = fma(u, u, h); }
        Ks[k * BAT_QT + lane] = kernel_tab<KT>(0.5 * h, lnc, T);
    }

    if (a.mean) {
        double m[BAT_MAX_O] = {};
        for (int k = 0; k < n; ++k) {
            const double kv = Ks[k * BAT_QT + lane];
#pragma unroll
            for (int o = 0; o < BAT_MAX_O; ++o)
                if (o < O) m[o] = fma(kv, al[k * O + o], m[o]);
        }
        if (valid) {
#pragma unroll
            for (int o = 0; o < BAT_MAX_O; ++o)
                if (o < O) a.mean[row * O + o] = m[o];
        }
    }
    if (DER && a.J) {
        // J[o][d] = sum_k k*_k (X_kd - x_d) / l_d^2 alpha_ko, a dimension at a time (its coordinates reread: no indexed registers)
        for (int d = 0; d < D; ++d) {
            const double ild = 1.0 / ls[a.n_ls == 1 ? 0 : d], xd = a.Xq[row * D + d] / ls[a.n_ls == 1 ? 0 : d];
            double jo[BAT_MAX_O] = {};
            for (int k = 0; k < n; ++k) {
                const double w = Ks[k * BAT_QT + lane] * ((Xl[k * D + d] - xd) * ild);
#pragma unroll
                for (int o = 0; o < BAT_MAX_O; ++o)
                    if (o < O) jo[o] = fma(w, al[k * O + o], jo[o]);
            }
            if (valid) {
#pragma unroll
                for (int o = 0; o < BAT_MAX_O; ++o)
                    if (o < O) a.J[(row * O + o) * D + d] = jo[o];
            }
        }
    }
    const bool der = DER && (a.Jvar || a.dvar);
    if (a.var || der) {
        double s0 = 0.0, sJ[DW] = {}, sD[DW] = {};
        for (int i = 0; i < n; ++i) {
            const double* __restrict__ wr = Wl + i * (i + 1) / 2;
            double a0 = 0.0;
            if (der) {
                double ad[DW] = {};
                for (int k = 0; k <= i; ++k) {
                    const double kv = Ks[k * BAT_QT + lane], w = wr[k];
                    a0 = fma(w, kv, a0);
                    const double wk = w * kv;
#pragma unroll
                    for (int d = 0; d < DW; ++d)
                        if (d < D) ad[d] = fma(wk, Xl[k * D + d] - xs[d], ad[d]);
                }
#pragma unroll
                for (int d = 0; d < DW; ++d) {
                    const double v = ad[d] * il[d];            // (W dk_d)_i: dk_d = k* (X_d - x_d) / l_d^2
                    sJ[d] = fma(v, v, sJ[d]);
                    sD[d] = fma(v, a0, sD[d]);
                }
            } else {
                for (int k = 0; k <= i; ++k) a0 = fma(wr[k], Ks[k * BAT_QT + lane], a0);
            }
            s0 = fma(a0, a0, s0);
        }
        if (valid) {
            if (a.var) a.var[row] = fmax((c + noise) - s0, 0.0);
#pragma unroll
            for (int d = 0; d < DW; ++d)
                if (d < D) {
                    if (DER && a.Jvar) a.Jvar[row * D + d] = c * il[d] * il[d] - sJ[d];
                    if (DER && a.dvar) a.dvar[row * D + d] = -2.0 * sD[d];
                }
        }
    }
}

template <int NMAX, bool OBJ>
void launch_factor(int ktype, int count, hipStream_t s, const BatArgs& a) {
    using Cfg = BatCfg<NMAX>;
    if (count < 1) return;
    with_kernel_type(ktype, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if constexpr (NMAX > BAT_SMALL_N) launch_lds<bat_factor<NMAX, KT, OBJ>>(dim3(count), dim3(Cfg::NT), Cfg::factor_lds, s, a);
        else hipLaunchKernelGGL((bat_factor<NMAX, KT, OBJ>), dim3(count), dim3(Cfg::NT), Cfg::factor_lds, s, a);
    });
}

template <int NMAX, int KT, bool DER, int DW>
void launch_predict_one(int tile0, int count, hipStream_t s, const BatPredArgs& a) {
    using Cfg = BatCfg<NMAX>;
    if constexpr (NMAX > BAT_SMALL_N) launch_lds<bat_predict<NMAX, KT, DER, DW>>(dim3(count), dim3(BAT_QT), Cfg::predict_lds, s, a, tile0);
    else hipLaunchKernelGGL((bat_predict<NMAX, KT, DER, DW>), dim3(count), dim3(BAT_QT), Cfg::predict_lds, s, a, tile0);
}

template <int NMAX>
void launch_predict(int ktype, bool der, int tile0, int count, hipStream_t s, const BatPredArgs& a) {
    if (count < 1) return;
    if (der) {                                                       // RBF only (checked by the entry point)
        with_coord_width(a.D, [&](auto dw) {
            constexpr int DW = decltype(dw)::value < MAX_DIMS ? decltype(dw)::value : MAX_DIMS;
            launch_predict_one<NMAX, KT_RBF, true, DW>(tile0, count, s, a);
        });
        return;
    }
    with_kernel_type(ktype, [&](auto kt) { launch_predict_one<NMAX, decltype(kt)::value, false, MAX_DIMS>(tile0, count, s, a); });
}

// One launch per size class present in the batch.
template <bool OBJ>
void launch_factor_classes(int ktype, int n_small, int n_large, hipStream_t s, BatArgs a) {
    launch_factor<BAT_SMALL_N, OBJ>(ktype, n_small, s, a);
    a.list += n_small;
    launch_factor<BAT_MAX_N, OBJ>(ktype, n_large, s, a);
}

}  // namespace

void launch_bat_factor(hipStream_t s, int ktype, bool obj, int n_small, int n_large, const BatArgs& a) {
    if (obj) launch_factor_classes<true>(ktype, n_small, n_large, s, a);
    else launch_factor_classes<false>(ktype, n_small, n_large, s, a);
}

void launch_bat_predict(hipStream_t s, int ktype, bool der, int tiles_small, int tiles_large, const BatPredArgs& a) {
    launch_predict<BAT_SMALL_N>(ktype, der, 0, tiles_small, s, a);
    launch_predict<BAT_MAX_N>(ktype, der, tiles_small, tiles_large, s, a);
}

}  // namespace gpt
