// A batch of independent small exact GPs (n <= 128 points each) — gpt_batch_lml_objective, gpt_batch_fit and
// gpt_batch_predict (include/gpt_hip.h).  The reference's transport problems are tiny and numerous (10 .. 20 source points per
// frame pair, hundreds of pairs); padded to 512 rows and factored by a chain of launches each of them costs what a 400-point
// model costs.  Here ONE workgroup owns one model from the Gram matrix to the gradient, and one launch serves every model of a
// size class (n <= 32: 64 threads and 12.5 KB of LDS, so many models share a CU; n <= 128: 256 threads and the 129-column image).
//
// bat_factor keeps the n x n image A in LDS with an odd row stride (column walks hit distinct banks):
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
#include "gpt_call.h"
#include "gpt_dispatch.h"
#include "gpt_exp.h"

#include <algorithm>

namespace gpt {
namespace {

constexpr int BAT_MAX_N = 128;           // points of one model
constexpr int BAT_SMALL_N = 32;          // ... of the small size class
constexpr int BAT_MAX_O = 16;            // outputs (right-hand sides)
constexpr int64_t BAT_MAX_B = 1 << 20;   // models of one call
constexpr int BAT_QT = 64;               // queries of a bat_predict workgroup = its threads
constexpr int BAT_RED = 4 + MAX_DIMS;    // values of the final reduction: y.alpha, sum log L_ii, d/dc, trace, d/dl_d

// One size class: threads, their TX x TY arrangement over a triangle, row stride of the image, dynamic LDS.
template <int NMAX> struct BatCfg {
    static constexpr int NT = NMAX <= BAT_SMALL_N ? 64 : 256;
    static constexpr int TX = NMAX <= BAT_SMALL_N ? 8 : 16;
    static constexpr int TY = NT / TX;
    static constexpr int LD = NMAX + 1;
    static constexpr int PER_THREAD = NMAX * BAT_MAX_O / NT;          // (point, output) pairs a thread owns
    static constexpr size_t factor_lds = ((size_t)NMAX * LD + (size_t)NMAX * BAT_MAX_O + NMAX) * sizeof(double);
    static constexpr int W_PACKED = NMAX * (NMAX + 1) / 2;
    static constexpr size_t predict_lds = ((size_t)W_PACKED + (size_t)NMAX * BAT_QT + (size_t)NMAX * MAX_DIMS + 256) * sizeof(double);
};

struct BatArgs {
    const double *X, *Y, *ls, *c, *noise;          // (rows, D), (rows, O), (B, n_ls), (B), (B)
    const int64_t *n_begin, *l_begin, *w_begin;    // (B + 1) each: rows, n^2 images, packed triangles before a model
    const int* list;                               // the models of this launch
    double *L, *alpha, *Wp, *lml, *grad;           // outputs; L, Wp, lml may be null; grad: objective only
    int* status;
    int D, O, n_ls;
    double jitter;
};

struct BatPredArgs {
    const double *X, *ls, *c, *noise, *alpha, *Wp, *Xq;
    const int64_t *n_begin, *w_begin, *q_begin;
    const int *tile_model, *tile_q0;               // per workgroup: the model, the first of its queries
    const int* status;
    double *mean, *var, *J, *Jvar, *dvar;          // any may be null
    int D, O, n_ls;
};

// c g(r) of dK/dlog l_d = c g(r) ((x_d - x'_d) / l_d)^2 (sklearn/gaussian_process/kernels.py:1568-1580, 1747-1778), beside
// kernel_libm's c k(r): RBF g = k, Matern 1/2 k / r, 3/2 3 e^{-sqrt3 r}, 5/2 5/3 (1 + sqrt5 r) e^{-sqrt5 r}
template <int KT>
__device__ __forceinline__ double kernel_libm_g(const double c, const double r2, const double kv) {
    if (KT == KT_RBF) return kv;
    const double r = sqrt(r2);
    if (KT == KT_MATERN12) return r > 0.0 ? kv / r : 0.0;
    if (KT == KT_MATERN32) return 3.0 * c * exp(-1.7320508075688772 * r);
    const double t = 2.23606797749979 * r;
    return (5.0 / 3.0) * c * (1.0 + t) * exp(-t);
}

// Sums of NV values over the workgroup, in a fixed order (butterfly inside a wave, then the waves in turn); every thread
// receives them.  Ends with a barrier: `red` may be reused at once.
template <int NT, int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*red)[NT / 64]) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double s = v[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (threadIdx.x % 64 == 0) red[q][threadIdx.x / 64] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double s = red[q][0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) s += red[q][w];
        v[q] = s;
    }
    __syncthreads();
}

template <int NMAX, int KT, bool OBJ>
__global__ __launch_bounds__(BatCfg<NMAX>::NT) void bat_factor(BatArgs a) {
    using Cfg = BatCfg<NMAX>;
    constexpr int NT = Cfg::NT, TX = Cfg::TX, TY = Cfg::TY, LD = Cfg::LD;
    extern __shared__ __attribute__((aligned(16))) double bat_lds[];
    double* __restrict__ A = bat_lds;                    // NMAX x LD
    double* __restrict__ buf = A + NMAX * LD;            // n x O: y, then W y, then alpha
    double* __restrict__ dinv = buf + NMAX * BAT_MAX_O;  // 1 / L_ii
    __shared__ double red[BAT_RED][NT / 64];

    const int b = a.list[blockIdx.x];
    const int64_t n0 = a.n_begin[b];
    const int n = (int)(a.n_begin[b + 1] - n0);
    const int D = a.D, O = a.O, tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const double c = a.c[b], noise = a.noise[b];
    const double* __restrict__ X = a.X + n0 * D;
    const double* __restrict__ Y = a.Y + n0 * O;
    double il[MAX_DIMS];
#pragma unroll
    for (int d = 0; d < MAX_DIMS; ++d) il[d] = d < D ? 1.0 / a.ls[(int64_t)b * a.n_ls + (a.n_ls == 1 ? 0 : d)] : 0.0;

    // K: sklearn's kernel_(X) with the WhiteKernel on the diagonal, then + alpha (_gpr.py:346-347)
    for (int i = ty; i < n; i += TY)
        for (int j = tx; j <= i; j += TX) {
            double kv = (c + noise) + a.jitter;
            if (i != j) {
                double r2 = 0.0;
#pragma unroll
                for (int d = 0; d < MAX_DIMS; ++d)
                    if (d < D) { const double u = (X[i * D + d] - X[j * D + d]) * il[d]; r2 = fma(u, u, r2); }
                kv = kernel_libm(KT, c, r2);
            }
            A[i * LD + j] = kv;
        }
    __syncthreads();

    // Cholesky, right-looking; the diagonal keeps the pivots until the end (nothing below reads it after its own column)
    for (int j = 0; j < n; ++j) {
        const double piv = A[j * LD + j];
        if (!(piv > 0.0)) {                       // the same LDS value in every thread: all of them leave
            if (tid == 0) a.status[b] = GPT_E_NOT_PD;
            return;
        }
        const double r = sqrt(piv);
        for (int i = j + 1 + tid; i < n; i += NT) A[i * LD + j] /= r;
        __syncthreads();
        for (int i = j + 1 + ty; i < n; i += TY) {
            const double lij = A[i * LD + j];
            for (int k = j + 1 + tx; k <= i; k += TX) A[i * LD + k] = fma(-lij, A[k * LD + j], A[i * LD + k]);
        }
        __syncthreads();
    }
    double sums[BAT_RED] = {};                     // [0] y.alpha  [1] sum log L_ii  [2] d/dc (off-diagonal)  [3] trace  [4 + d] d/dl_d
    for (int i = tid; i < n; i += NT) {
        const double l = sqrt(A[i * LD + i]);
        A[i * LD + i] = l;
        dinv[i] = 1.0 / l;
        sums[1] += log(l);
    }
    __syncthreads();

    // W = L^-1, row by row, W_ij kept at A[j][i]:  W_ij = -(sum_{k=j}^{i-1} L_ik W_kj) / L_ii
    for (int i = 1; i < n; ++i) {
        for (int j = tid; j < i; j += NT) {
            double s = A[i * LD + j] * dinv[j];
            for (int k = i - 1; k > j; --k) s = fma(A[i * LD + k], A[j * LD + k], s);
            A[j * LD + i] = -s * dinv[i];
        }
        __syncthreads();
    }

    // alpha = W^T (W y): each thread owns up to PER_THREAD (point, output) pairs and carries them over the two barriers
    const int nO = n * O;
    for (int e = tid; e < nO; e += NT) buf[e] = Y[e];
    __syncthreads();
    double reg[Cfg::PER_THREAD];
#pragma unroll
    for (int u = 0; u < Cfg::PER_THREAD; ++u) {
        const int e = tid + u * NT;
        reg[u] = 0.0;
        if (e < nO) {
            const int i = e / O, o = e - i * O;
            double s = 0.0;
            for (int k = 0; k < i; ++k) s = fma(A[k * LD + i], buf[k * O + o], s);
            reg[u] = fma(dinv[i], buf[e], s);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Cfg::PER_THREAD; ++u) {
        const int e = tid + u * NT;
        if (e < nO) buf[e] = reg[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Cfg::PER_THREAD; ++u) {
        const int e = tid + u * NT;
        if (e < nO) {
            const int i = e / O, o = e - i * O;
            double s = dinv[i] * buf[e];
            for (int k = i + 1; k < n; ++k) s = fma(A[i * LD + k], buf[k * O + o], s);
            reg[u] = s;
            sums[0] = fma(Y[e], s, sums[0]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < Cfg::PER_THREAD; ++u) {
        const int e = tid + u * NT;
        if (e < nO) {
            buf[e] = reg[u];
            if (!OBJ) a.alpha[n0 * O + e] = reg[u];
        }
    }
    __syncthreads();

    if (!OBJ) {
        if (a.L) {
            double* __restrict__ Lg = a.L + a.l_begin[b];
            for (int i = ty; i < n; i += TY)
                for (int j = tx; j < n; j += TX) Lg[i * n + j] = j <= i ? A[i * LD + j] : 0.0;
        }
        if (a.Wp) {
            double* __restrict__ Wg = a.Wp + a.w_begin[b];
            for (int i = ty; i < n; i += TY)
                for (int j = tx; j <= i; j += TX) Wg[i * (i + 1) / 2 + j] = j < i ? A[j * LD + i] : dinv[i];
        }
    }

    if (OBJ) {
        // 1/2 tr((alpha alpha^T - O K^-1) dK/dtheta): the strict lower triangle counts twice, dK/dtheta from the coordinates
        for (int i = ty; i < n; i += TY)
            for (int j = tx; j <= i; j += TX) {
                double kin = i == j ? dinv[i] * dinv[i] : dinv[i] * A[j * LD + i];
                for (int k = i + 1; k < n; ++k) kin = fma(A[i * LD + k], A[j * LD + k], kin);
                double aa = 0.0;
                for (int o = 0; o < O; ++o) aa = fma(buf[i * O + o], buf[j * O + o], aa);
                const double inner = aa - (double)O * kin;
                if (i == j) { sums[3] += inner; continue; }
                double r2 = 0.0;
#pragma unroll
                for (int d = 0; d < MAX_DIMS; ++d)
                    if (d < D) { const double u = (X[i * D + d] - X[j * D + d]) * il[d]; r2 = fma(u, u, r2); }
                const double kv = kernel_libm(KT, c, r2);
                const double wg = inner * kernel_libm_g<KT>(c, r2, kv);
                sums[2] = fma(inner, kv, sums[2]);
                if (a.n_ls == 1) sums[4] = fma(wg, r2, sums[4]);
                else {
#pragma unroll
                    for (int d = 0; d < MAX_DIMS; ++d)
                        if (d < D) { const double u = (X[i * D + d] - X[j * D + d]) * il[d]; sums[4 + d] = fma(wg, u * u, sums[4 + d]); }
                }
            }
        block_sum<NT, BAT_RED>(sums, red);
    } else {
        double two[2] = {sums[0], sums[1]};
        block_sum<NT, 2>(two, red);
        sums[0] = two[0]; sums[1] = two[1];
    }
    if (tid == 0) {
        const double lml = -0.5 * sums[0] - (double)O * sums[1] - (double)O * (0.5 * n) * 1.8378770664093453;   // log(2 pi)
        if (a.lml) a.lml[b] = lml;
        if (OBJ) {
            double* __restrict__ g = a.grad + (int64_t)b * (2 + a.n_ls);
            g[0] = sums[2] + 0.5 * c * sums[3];
#pragma unroll
            for (int d = 0; d < MAX_DIMS; ++d)
                if (d < a.n_ls) g[1 + d] = sums[4 + d];
            g[1 + a.n_ls] = 0.5 * noise * sums[3];
        }
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

// What the three entry points share: the validated batch and the prefix sums the kernels index by.
struct Batch {
    int64_t B = 0, rows = 0, l_total = 0, w_total = 0;
    int n_small = 0;                      // models of the small size class; they come first in `list`
    std::vector<int64_t> l_begin, w_begin;
    std::vector<int> list;
};

int check_batch(const std::string& w, Batch& bt, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                const double* ls, int n_ls, const double* c, const double* noise, double jitter, int ktype, const int* status) {
    if (!X || !Y || !n_begin || !ls || !c || !noise || !status) return fail(GPT_E_ARG, w + ": NULL argument");
    if (B < 1 || B > BAT_MAX_B) return fail(GPT_E_ARG, w + ": B (models) must be 1 .. 2^20, got " + std::to_string(B));
    if (D < 1 || D > MAX_DIMS) return fail(GPT_E_ARG, w + ": D must be 1 .. 15, got " + std::to_string(D));
    if (O < 1 || O > BAT_MAX_O) return fail(GPT_E_ARG, w + ": O (outputs) must be 1 .. 16, got " + std::to_string(O));
    if (n_ls != 1 && n_ls != D) return fail(GPT_E_ARG, w + ": n_ls must be 1 or D");
    if (ktype < GPT_KERNEL_RBF || ktype > GPT_KERNEL_MATERN52) return fail(GPT_E_ARG, w + ": unknown kernel_type");
    if (!(jitter >= 0) || !std::isfinite(jitter)) return fail(GPT_E_ARG, w + ": alpha_jitter must be finite and >= 0");
    if (n_begin[0] != 0) return fail(GPT_E_ARG, w + ": n_begin[0] must be 0");
    bt.B = B;
    bt.l_begin.assign(B + 1, 0);
    bt.w_begin.assign(B + 1, 0);
    bt.list.resize(B);
    std::vector<int> large;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = n_begin[b + 1] - n_begin[b];
        if (n < 1 || n > BAT_MAX_N)
            return fail(GPT_E_ARG, w + ": every model needs 1 <= n_b <= 128 points with increasing offsets; model " + std::to_string(b) +
                                       " has n_begin " + std::to_string(n_begin[b]) + " .. " + std::to_string(n_begin[b + 1]));
        bt.l_begin[b + 1] = bt.l_begin[b] + n * n;
        bt.w_begin[b + 1] = bt.w_begin[b] + n * (n + 1) / 2;
        if (n <= BAT_SMALL_N) bt.list[bt.n_small++] = (int)b;
        else large.push_back((int)b);
    }
    std::copy(large.begin(), large.end(), bt.list.begin() + bt.n_small);
    bt.rows = n_begin[B];
    bt.l_total = bt.l_begin[B];
    bt.w_total = bt.w_begin[B];
    if (!all_finite(X, (size_t)bt.rows * D) || !all_finite(Y, (size_t)bt.rows * O))
        return fail(GPT_E_ARG, w + ": X or Y contains NaN or infinity");
    for (int64_t e = 0; e < B * n_ls; ++e)
        if (!(ls[e] > 0) || !std::isfinite(ls[e])) return fail(GPT_E_ARG, w + ": length_scale must be finite and > 0 (model " + std::to_string(e / n_ls) + ")");
    for (int64_t b = 0; b < B; ++b)
        if (!(c[b] > 0) || !std::isfinite(c[b]) || !(noise[b] >= 0) || !std::isfinite(noise[b]))
            return fail(GPT_E_ARG, w + ": need finite constant_value > 0 and noise_level >= 0 (model " + std::to_string(b) + ")");
    return GPT_OK;
}

// Device image of a call's inputs: one buffer of doubles and one of integers, one copy each.
struct BatDevice {
    double *X, *Y, *ls, *c, *noise, *Xq = nullptr;
    int64_t *n_begin, *l_begin, *w_begin, *q_begin = nullptr;
    int *list, *tile_model = nullptr, *tile_q0 = nullptr;
};

int upload(CallBuffers& buf, BatDevice& dv, const Batch& bt, const double* X, const double* Y, const int64_t* n_begin, int D, int O,
           const double* ls, int n_ls, const double* c, const double* noise, const double* Xq, const int64_t* q_begin,
           const std::vector<int>& tile_model, const std::vector<int>& tile_q0) {
    const size_t B = (size_t)bt.B, nx = (size_t)bt.rows * D, ny = (size_t)bt.rows * O, nq = q_begin ? (size_t)q_begin[B] * D : 0;
    std::vector<double> hd;
    hd.reserve(nx + ny + B * (n_ls + 2) + nq);
    hd.insert(hd.end(), X, X + nx);
    hd.insert(hd.end(), Y, Y + ny);
    hd.insert(hd.end(), ls, ls + B * n_ls);
    hd.insert(hd.end(), c, c + B);
    hd.insert(hd.end(), noise, noise + B);
    if (nq) hd.insert(hd.end(), Xq, Xq + nq);
    const size_t nt = tile_model.size();
    std::vector<int64_t> hi(4 * (B + 1) + (B + 2 * nt + 1) / 2 + 1, 0);
    std::copy(n_begin, n_begin + B + 1, hi.begin());
    std::copy(bt.l_begin.begin(), bt.l_begin.end(), hi.begin() + (B + 1));
    std::copy(bt.w_begin.begin(), bt.w_begin.end(), hi.begin() + 2 * (B + 1));
    if (q_begin) std::copy(q_begin, q_begin + B + 1, hi.begin() + 3 * (B + 1));
    int* h32 = reinterpret_cast<int*>(hi.data() + 4 * (B + 1));
    std::copy(bt.list.begin(), bt.list.end(), h32);
    std::copy(tile_model.begin(), tile_model.end(), h32 + B);
    std::copy(tile_q0.begin(), tile_q0.end(), h32 + B + nt);

    double* dd;
    int64_t* di;
    CALLCHK(buf.alloc(&dd, hd.size()));
    CALLCHK(buf.alloc(&di, hi.size()));
    CALLCHK(hipMemcpyAsync(dd, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipMemcpyAsync(di, hi.data(), hi.size() * sizeof(int64_t), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));          // the staging vectors end with this function
    dv.X = dd; dv.Y = dv.X + nx; dv.ls = dv.Y + ny; dv.c = dv.ls + B * n_ls; dv.noise = dv.c + B; dv.Xq = dv.noise + B;
    dv.n_begin = di; dv.l_begin = di + (B + 1); dv.w_begin = di + 2 * (B + 1); dv.q_begin = di + 3 * (B + 1);
    dv.list = reinterpret_cast<int*>(di + 4 * (B + 1));
    dv.tile_model = dv.list + B;
    dv.tile_q0 = dv.tile_model + nt;
    return GPT_OK;
}

BatArgs factor_args(const BatDevice& dv, int D, int O, int n_ls, double jitter) {
    BatArgs a{};
    a.X = dv.X; a.Y = dv.Y; a.ls = dv.ls; a.c = dv.c; a.noise = dv.noise;
    a.n_begin = dv.n_begin; a.l_begin = dv.l_begin; a.w_begin = dv.w_begin; a.list = dv.list;
    a.D = D; a.O = O; a.n_ls = n_ls; a.jitter = jitter;
    return a;
}

// One launch per size class present in the batch.
template <bool OBJ>
void launch_factor_classes(const Batch& bt, int ktype, hipStream_t s, BatArgs a) {
    launch_factor<BAT_SMALL_N, OBJ>(ktype, bt.n_small, s, a);
    a.list += bt.n_small;
    launch_factor<BAT_MAX_N, OBJ>(ktype, (int)(bt.B - bt.n_small), s, a);
}

// dst[begin[b] * width ..] = src[...] for every model whose status is GPT_OK (a failed model's outputs stay untouched)
void scatter_ok(double* dst, const double* src, const int64_t* begin, size_t width, const int* status, int64_t B) {
    if (!dst) return;
    for (int64_t b = 0; b < B; ++b)
        if (status[b] == GPT_OK)
            std::copy(src + (size_t)begin[b] * width, src + (size_t)begin[b + 1] * width, dst + (size_t)begin[b] * width);
}

}  // namespace
}  // namespace gpt

using namespace gpt;

extern "C" int gpt_batch_lml_objective(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                                       const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                                       double alpha_jitter, int kernel_type, double* lml, double* grad, int* status) {
    const std::string w = "gpt_batch_lml_objective";
    if (!lml || !grad) return fail(GPT_E_ARG, w + ": NULL argument");
    Batch bt;
    if (int rc = check_batch(w, bt, X, Y, n_begin, B, D, O, length_scale, n_ls, constant_value, noise_level, alpha_jitter, kernel_type, status))
        return rc;
    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    BatDevice dv;
    if (int rc = upload(buf, dv, bt, X, Y, n_begin, D, O, length_scale, n_ls, constant_value, noise_level, nullptr, nullptr, {}, {})) return rc;
    const size_t G = 2 + n_ls, nout = (size_t)B * (1 + G) + ((size_t)B + 1) / 2;      // lml | grad | status (int)
    double* dout;
    CALLCHK(buf.alloc(&dout, nout));
    BatArgs a = factor_args(dv, D, O, n_ls, alpha_jitter);
    a.lml = dout; a.grad = dout + B; a.status = reinterpret_cast<int*>(dout + (size_t)B * (1 + G));
    launch_factor_classes<true>(bt, kernel_type, buf.stream, a);
    CALLCHK(hipGetLastError());
    std::vector<double> out(nout);
    CALLCHK(hipMemcpyAsync(out.data(), dout, nout * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));
    const int* st = reinterpret_cast<const int*>(out.data() + (size_t)B * (1 + G));
    for (int64_t b = 0; b < B; ++b) {
        status[b] = st[b];
        if (st[b] != GPT_OK) continue;
        lml[b] = out[b];
        std::copy(out.begin() + B + b * G, out.begin() + B + (b + 1) * G, grad + b * G);
    }
    return GPT_OK;
}

extern "C" int gpt_batch_fit(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                             const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                             double alpha_jitter, int kernel_type, double* L, double* alpha, double* lml, int* status) {
    const std::string w = "gpt_batch_fit";
    if (!alpha) return fail(GPT_E_ARG, w + ": NULL argument");
    Batch bt;
    if (int rc = check_batch(w, bt, X, Y, n_begin, B, D, O, length_scale, n_ls, constant_value, noise_level, alpha_jitter, kernel_type, status))
        return rc;
    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    BatDevice dv;
    if (int rc = upload(buf, dv, bt, X, Y, n_begin, D, O, length_scale, n_ls, constant_value, noise_level, nullptr, nullptr, {}, {})) return rc;
    const size_t na = (size_t)bt.rows * O, nl = L ? (size_t)bt.l_total : 0, nout = (size_t)B + na + nl + ((size_t)B + 1) / 2;
    double* dout;                                                                     // lml | alpha | L | status (int)
    CALLCHK(buf.alloc(&dout, nout));
    BatArgs a = factor_args(dv, D, O, n_ls, alpha_jitter);
    a.lml = dout; a.alpha = dout + B; a.L = L ? dout + B + na : nullptr; a.status = reinterpret_cast<int*>(dout + B + na + nl);
    launch_factor_classes<false>(bt, kernel_type, buf.stream, a);
    CALLCHK(hipGetLastError());
    std::vector<double> out(nout);
    CALLCHK(hipMemcpyAsync(out.data(), dout, nout * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));
    const int* st = reinterpret_cast<const int*>(out.data() + B + na + nl);
    std::copy(st, st + B, status);
    if (lml)
        for (int64_t b = 0; b < B; ++b)
            if (st[b] == GPT_OK) lml[b] = out[b];
    scatter_ok(alpha, out.data() + B, n_begin, O, st, B);
    scatter_ok(L, out.data() + B + na, bt.l_begin.data(), 1, st, B);
    return GPT_OK;
}

extern "C" int gpt_batch_predict(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                                 const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                                 double alpha_jitter, int kernel_type, const double* Xq, const int64_t* q_begin, double* mean, double* var,
                                 double* J, double* Jvar, double* dvar, int* status) {
    const std::string w = "gpt_batch_predict";
    if (!q_begin) return fail(GPT_E_ARG, w + ": NULL argument");
    Batch bt;
    if (int rc = check_batch(w, bt, X, Y, n_begin, B, D, O, length_scale, n_ls, constant_value, noise_level, alpha_jitter, kernel_type, status))
        return rc;
    const bool der = J || Jvar || dvar;
    if (der && kernel_type != GPT_KERNEL_RBF)
        return fail(GPT_E_ARG, w + ": J, Jvar and dvar are RBF only in a batch (the analytic Matern derivatives: GaussianProcess(matern_derivatives=True))");
    if (q_begin[0] != 0) return fail(GPT_E_ARG, w + ": q_begin[0] must be 0");
    for (int64_t b = 0; b < B; ++b)
        if (q_begin[b + 1] < q_begin[b] || q_begin[b + 1] > INT_MAX)
            return fail(GPT_E_ARG, w + ": q_begin must not decrease (M_b >= 0) and the queries of a call must number fewer than 2^31 (model " +
                                       std::to_string(b) + ")");
    const int64_t M = q_begin[B];
    if (M > 0 && !Xq) return fail(GPT_E_ARG, w + ": NULL argument");
    if (M > 0 && !all_finite(Xq, (size_t)M * D)) return fail(GPT_E_ARG, w + ": Xq contains NaN or infinity");
    // tiles of 64 queries, in the order of bt.list: the small size class first
    std::vector<int> tile_model, tile_q0;
    int tiles_small = 0;
    for (int64_t k = 0; k < B; ++k) {
        const int b = bt.list[k];
        for (int64_t q0 = 0; q0 < q_begin[b + 1] - q_begin[b]; q0 += BAT_QT) { tile_model.push_back(b); tile_q0.push_back((int)q0); }
        if (k + 1 == bt.n_small) tiles_small = (int)tile_model.size();
    }
    if (bt.n_small == 0) tiles_small = 0;
    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    BatDevice dv;
    if (int rc = upload(buf, dv, bt, X, Y, n_begin, D, O, length_scale, n_ls, constant_value, noise_level, Xq, q_begin, tile_model, tile_q0))
        return rc;
    // scratch of the factor: alpha | packed W | status; then the outputs asked for
    const size_t na = (size_t)bt.rows * O;
    double *dfac, *dout;
    CALLCHK(buf.alloc(&dfac, na + (size_t)bt.w_total + ((size_t)B + 1) / 2));
    const size_t widths[5] = {mean ? (size_t)O : 0, var ? (size_t)1 : 0, J ? (size_t)O * D : 0, Jvar ? (size_t)D : 0, dvar ? (size_t)D : 0};
    size_t off[6] = {0};
    for (int k = 0; k < 5; ++k) off[k + 1] = off[k] + widths[k] * (size_t)M;
    CALLCHK(buf.alloc(&dout, off[5]));
    BatArgs a = factor_args(dv, D, O, n_ls, alpha_jitter);
    a.alpha = dfac; a.Wp = dfac + na; a.status = reinterpret_cast<int*>(dfac + na + bt.w_total);
    launch_factor_classes<false>(bt, kernel_type, buf.stream, a);
    BatPredArgs p{};
    p.X = dv.X; p.ls = dv.ls; p.c = dv.c; p.noise = dv.noise; p.alpha = a.alpha; p.Wp = a.Wp; p.Xq = dv.Xq;
    p.n_begin = dv.n_begin; p.w_begin = dv.w_begin; p.q_begin = dv.q_begin; p.tile_model = dv.tile_model; p.tile_q0 = dv.tile_q0;
    p.status = a.status; p.D = D; p.O = O; p.n_ls = n_ls;
    p.mean = mean ? dout + off[0] : nullptr; p.var = var ? dout + off[1] : nullptr; p.J = J ? dout + off[2] : nullptr;
    p.Jvar = Jvar ? dout + off[3] : nullptr; p.dvar = dvar ? dout + off[4] : nullptr;
    if (off[5] > 0) {
        launch_predict<BAT_SMALL_N>(kernel_type, der, 0, tiles_small, buf.stream, p);
        launch_predict<BAT_MAX_N>(kernel_type, der, tiles_small, (int)tile_model.size() - tiles_small, buf.stream, p);
    }
    CALLCHK(hipGetLastError());
    std::vector<double> out(off[5]);
    std::vector<int> st(B);
    CALLCHK(hipMemcpyAsync(st.data(), a.status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, buf.stream));
    if (off[5] > 0) CALLCHK(hipMemcpyAsync(out.data(), dout, off[5] * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));
    std::copy(st.begin(), st.end(), status);
    double* dst[5] = {mean, var, J, Jvar, dvar};
    for (int k = 0; k < 5; ++k) scatter_ok(dst[k], out.data() + off[k], q_begin, widths[k], st.data(), B);
    return GPT_OK;
}
