// Device code of the batched small-GP unit outside its kernels (internal header, device halves only): the size classes, the
// workgroup sum, and one model's factorisation from the Gram matrix to the reduced sums of the LML and its gradient as a function,
// bat_factor_body, with the LML and the gradient assembled from those sums (bat_lml, bat_grad).  It is the only text of that
// computation: bat_factor (gpt_batch.hip) calls it once per model, bat_optimize (gpt_batch_opt.hip) once per objective evaluation
// of a run, so the search optimises exactly what gpt_batch_lml_objective and gpt_batch_fit report.  The order of its statements,
// barriers and sums is what the bit-for-bit independence of a model from its batch rests on.  The image and the summation orders
// are described at the top of gpt_batch.hip.
#pragma once
#include "gpt_batch.h"
#include "gpt_exp.h"

namespace gpt {

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

// One model b (rows n0 .. n0 + n) at the hyper-parameters (c, il = 1 / length-scale per dimension, noise): the image in A, alpha
// in buf, 1 / L_ii in dinv, and in every thread the reduced sums
//     [0] y.alpha  [1] sum log L_ii  and, OBJ only,  [2] d/dc (off-diagonal)  [3] trace  [4 + d] d/dl_d.
// !OBJ also writes a.alpha and whichever of a.L, a.Wp are not null.  Returns false at a pivot that is not positive: the pivot is
// the same LDS value in every thread, so all of them return there together, after the same barriers, with nothing written to
// global memory.  `sums` comes in uninitialised and is zeroed here, after the Cholesky loop: zeroed by the caller its BAT_RED
// values would stay live in registers through the Gram and Cholesky loops.
template <int NMAX, int KT, bool OBJ>
__device__ __forceinline__ bool bat_factor_body(const BatArgs& a, const int b, const int64_t n0, const int n, const double c, const double noise,
                                                const double (&il)[MAX_DIMS], double* __restrict__ A, double* __restrict__ buf,
                                                double* __restrict__ dinv, double (*red)[BatCfg<NMAX>::NT / 64], double (&sums)[BAT_RED]) {
    using Cfg = BatCfg<NMAX>;
    constexpr int NT = Cfg::NT, TX = Cfg::TX, TY = Cfg::TY, LD = Cfg::LD;
    const int D = a.D, O = a.O, tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
    const double* __restrict__ X = a.X + n0 * D;
    const double* __restrict__ Y = a.Y + n0 * O;

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
        if (!(piv > 0.0)) return false;           // the same LDS value in every thread: all of them leave
        const double r = sqrt(piv);
        for (int i = j + 1 + tid; i < n; i += NT) A[i * LD + j] /= r;
        __syncthreads();
        for (int i = j + 1 + ty; i < n; i += TY) {
            const double lij = A[i * LD + j];
            for (int k = j + 1 + tx; k <= i; k += TX) A[i * LD + k] = fma(-lij, A[k * LD + j], A[i * LD + k]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < BAT_RED; ++q) sums[q] = 0.0;
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
    return true;
}

// LML from the reduced sums of bat_factor_body
__device__ __forceinline__ double bat_lml(const double (&sums)[BAT_RED], const int n, const int O) {
    return -0.5 * sums[0] - (double)O * sums[1] - (double)O * (0.5 * n) * 1.8378770664093453;   // log(2 pi)
}

// ... and its gradient by theta = log [c, l (n_ls of them), noise] into g[0 .. 2 + n_ls)
__device__ __forceinline__ void bat_grad(const double (&sums)[BAT_RED], const double c, const double noise, const int n_ls, double* __restrict__ g) {
    g[0] = sums[2] + 0.5 * c * sums[3];
#pragma unroll
    for (int d = 0; d < MAX_DIMS; ++d)
        if (d < n_ls) g[1 + d] = sums[4 + d];
    g[1 + n_ls] = 0.5 * noise * sums[3];
}

}  // namespace gpt
