// D x D algebra of the transport units, D <= 3 (device units only): determinant, products and the affine part gamma, each
// force-inlined and unrolled so that everything stays in registers, and the run-time D -> Int<D> dispatch.  A
// matrix operand is a register array double[D][D] or a row-major pointer, a vector operand an array or a pointer — the kernels
// keep some operands in registers and read others straight from their arguments; both are taken by value, an array as the
// pointer it decays to.  The operation order is part of the contract (the
// results are compared bit for bit across kernels): every sum starts with a plain product and goes on with fma in index order.
#pragma once
#include "gpt_dispatch.h"

namespace gpt {

template <int D> __device__ __forceinline__ double sm_el(const double (*A)[D], const int i, const int j) { return A[i][j]; }
template <int D> __device__ __forceinline__ double sm_el(const double* A, const int i, const int j) { return (A + i * D)[j]; }

template <int D> __device__ __forceinline__ double sm_det(const double (&A)[D][D]) {
    if constexpr (D == 1) return A[0][0];
    else if constexpr (D == 2) return A[0][0] * A[1][1] - A[0][1] * A[1][0];
    else return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// (A v)[i]
template <int D, class M, class V> __device__ __forceinline__ double sm_row_dot(const M A, const int i, const V v) {
    double r = sm_el<D>(A, i, 0) * v[0];
#pragma unroll
    for (int d = 1; d < D; ++d) r = fma(sm_el<D>(A, i, d), v[d], r);
    return r;
}
// (A^T v)[i], the products taken as v[d] A[d][i]
template <int D, class M, class V> __device__ __forceinline__ double sm_col_dot(const V v, const M A, const int i) {
    double r = v[0] * sm_el<D>(A, 0, i);
#pragma unroll
    for (int d = 1; d < D; ++d) r = fma(v[d], sm_el<D>(A, d, i), r);
    return r;
}
// (A B)[o][e]
template <int D, class MA, class MB> __device__ __forceinline__ double sm_mat_el(const MA A, const MB B, const int o, const int e) {
    double b = sm_el<D>(A, o, 0) * sm_el<D>(B, 0, e);
#pragma unroll
    for (int d = 1; d < D; ++d) b = fma(sm_el<D>(A, o, d), sm_el<D>(B, d, e), b);
    return b;
}

// out = A v, row by row: `out` may be memory that the operands alias
template <int D, class M, class V, class O> __device__ __forceinline__ void sm_mat_vec(const M A, const V v, const O out) {
#pragma unroll
    for (int i = 0; i < D; ++i) out[i] = sm_row_dot<D>(A, i, v);
}

// C = A B
template <int D, class MA, class MB> __device__ __forceinline__ void sm_mat_mat(const MA A, const MB B, double (&C)[D][D]) {
#pragma unroll
    for (int o = 0; o < D; ++o)
#pragma unroll
        for (int e = 0; e < D; ++e) C[o][e] = sm_mat_el<D>(A, B, o, e);
}

// The affine part of a transport: `t` is anything with the members c_src, c_dst (pointers) and scale; R, the (D,D) rotation, is
// passed apart, since a kernel that applies it twice keeps it in registers.
// g = gamma(x) = scale R (x - c_src) + c_dst, row by row as sm_mat_vec
template <int D, class T, class M, class V, class O>
__device__ __forceinline__ void sm_affine(const T& t, const M R, const V x, const O g) {
    double xc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xc[d] = x[d] - t.c_src[d];
#pragma unroll
    for (int i = 0; i < D; ++i) g[i] = fma(t.scale, sm_row_dot<D>(R, i, xc), t.c_dst[i]);
}

// f(Int<D>{}) for the D <= 3 of the transport
template <class F> void with_small_dim(int D, F&& f) {
    switch (D) {
        case 1: f(Int<1>{}); break;
        case 2: f(Int<2>{}); break;
        default: f(Int<3>{});
    }
}

}  // namespace gpt
