// Epilogue of the transport for gfx950 (MI355X): what PolicyTransportation.transport / transport_velocity /
// transport_orientation (policy_transportation.py:30-75 of the reference) do on the host around the posterior, done where the
// posterior already is.  Two kernels around the existing launches (launch_mean_jac / launch_var, unchanged):
//
//  k_affine       : pos -> gamma(pos) = scale R (pos - c_src) + c_dst, the query image of the posterior launches.
//  k_push_forward : one thread per query, plain fp64 FMA, no LDS.  pos_out = gamma(pos) + mean; vel_out = (I + J) R_jac vel with
//               its variance sum_d Jvar_d (R_jac vel)_d^2 and det((I + J) R_jac); and, D = 3, the rotation closest to
//               J' = (I + J(pos)) R_jac as a quaternion times the demonstration's: Bar-Itzhack's symmetric 4 x 4 matrix K(J'),
//               its dominant eigenvector by cyclic Jacobi — TRANSPORT_JACOBI_SWEEPS sweeps over the six (p,q) pairs, every
//               index a compile-time constant so that K and V (26 doubles) stay in registers, no convergence test — taken as
//               the column of the largest diagonal entry (lowest index on a tie), normalised, sign w >= 0.
//               A query's result depends on its own row alone.
#include "gpt_transport.h"
#include "gpt_small.h"

namespace gpt {

template <int D>
__global__ __launch_bounds__(256) void k_affine(TransportArgs a) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.M) return;
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = a.pos[m * D + d] - a.c_src[d];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        // (sm_affine's statement, kept here: through the helper the D = 3 instantiation merges its loads of R in another order)
        a.pos_rot[m * D + i] = fma(a.scale, sm_row_dot<D>(a.R, i, x), a.c_dst[i]);
    }
}

// B = (I + J[m]) Rj
template <int D>
__device__ __forceinline__ void tp_jacobian(const double* __restrict__ J, const int64_t m, const double (&Rj)[D][D], double (&B)[D][D]) {
    double A[D][D];
#pragma unroll
    for (int o = 0; o < D; ++o)
#pragma unroll
        for (int d = 0; d < D; ++d) A[o][d] = (o == d ? 1.0 : 0.0) + J[(m * D + o) * D + d];
    sm_mat_mat<D>(A, Rj, B);
}

// One Jacobi rotation in the (P,Q) plane of the symmetric K (both triangles kept), accumulated into V's columns.
// t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (K_qq - K_pp) / (2 K_pq): the smaller root, |t| <= 1.  K_pq == 0: no
// rotation.  theta^2 overflowing gives t = 0; a NaN anywhere gives NaN.
template <int P, int Q> __device__ __forceinline__ void tp_rotate(double (&K)[4][4], double (&V)[4][4]) {
    const double apq = K[P][Q];
    const double theta = (K[Q][Q] - K[P][P]) / (2.0 * apq);
    double t = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
    t = apq == 0.0 ? 0.0 : t;
    const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c, tau = s / (1.0 + c);
    const double h = t * apq;
    K[P][P] -= h;
    K[Q][Q] += h;
    K[P][Q] = K[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double g = K[r][P], f = K[r][Q];
            K[r][P] = K[P][r] = g - s * fma(tau, g, f);
            K[r][Q] = K[Q][r] = f + s * fma(-tau, f, g);
        }
        const double g = V[r][P], f = V[r][Q];
        V[r][P] = g - s * fma(tau, g, f);
        V[r][Q] = f + s * fma(-tau, f, g);
    }
}

// Bar-Itzhack (2000): the unit quaternion of the rotation closest to B is the dominant eigenvector, (x, y, z, w), of K(B).
// Returns q = (w, x, y, z) with w >= 0 and gap = (lambda_4 - lambda_3) / |K|_F.
__device__ __forceinline__ void tp_quaternion(const double (&B)[3][3], double (&q)[4], double& gap) {
    constexpr double T = 1.0 / 3.0;
    double K[4][4], V[4][4];
    K[0][0] = (B[0][0] - B[1][1] - B[2][2]) * T;
    K[1][1] = (B[1][1] - B[0][0] - B[2][2]) * T;
    K[2][2] = (B[2][2] - B[0][0] - B[1][1]) * T;
    K[3][3] = (B[0][0] + B[1][1] + B[2][2]) * T;
    K[0][1] = K[1][0] = (B[1][0] + B[0][1]) * T;
    K[0][2] = K[2][0] = (B[2][0] + B[0][2]) * T;
    K[1][2] = K[2][1] = (B[2][1] + B[1][2]) * T;
    K[0][3] = K[3][0] = (B[2][1] - B[1][2]) * T;
    K[1][3] = K[3][1] = (B[0][2] - B[2][0]) * T;
    K[2][3] = K[3][2] = (B[1][0] - B[0][1]) * T;
    double f2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f2 = fma(K[i][j], K[i][j], f2);
            V[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < TRANSPORT_JACOBI_SWEEPS; ++sweep) {
        tp_rotate<0, 1>(K, V);
        tp_rotate<0, 2>(K, V);
        tp_rotate<0, 3>(K, V);
        tp_rotate<1, 2>(K, V);
        tp_rotate<1, 3>(K, V);
        tp_rotate<2, 3>(K, V);
    }
    // the largest diagonal entry (lowest index on a tie) and the one below it, by selects: no run-time index into K or V
    double lam = K[0][0], lam2 = -__builtin_inf(), v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = V[r][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const double x = K[i][i];
        const bool up = x > lam;
        lam2 = up ? lam : (x > lam2 ? x : lam2);
        lam = up ? x : lam;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = up ? V[r][i] : v[r];
    }
    gap = (lam - lam2) / sqrt(f2);
    const double n2 = fma(v[3], v[3], fma(v[2], v[2], fma(v[1], v[1], v[0] * v[0])));
    const double inv = (v[3] < 0.0 ? -1.0 : 1.0) / sqrt(n2);
    q[0] = v[3] * inv; q[1] = v[0] * inv; q[2] = v[1] * inv; q[3] = v[2] * inv;
}

template <int D>
__global__ __launch_bounds__(256) void k_push_forward(TransportArgs a) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.M) return;
    double Rj[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int d = 0; d < D; ++d) Rj[i][d] = a.R_jac[i * D + d];
#pragma unroll
    for (int d = 0; d < D; ++d) a.pos_out[m * D + d] = a.pos_rot[m * D + d] + a.mean[m * D + d];
    if (a.det_vel) {
        double B[D][D];
        tp_jacobian<D>(a.J, m, Rj, B);
        a.det_vel[m] = sm_det<D>(B);
    }
    if (a.vel_out || a.vel_var) {
        double vr[D];                              // R_jac vel
#pragma unroll
        for (int i = 0; i < D; ++i) {
            vr[i] = sm_row_dot<D>(Rj, i, a.vel + m * D);
        }
        if (a.vel_out) {
#pragma unroll
            for (int o = 0; o < D; ++o) {
                double r = vr[o];
#pragma unroll
                for (int d = 0; d < D; ++d) r = fma(a.J[(m * D + o) * D + d], vr[d], r);
                a.vel_out[m * D + o] = r;
            }
        }
        if (a.vel_var) {
            double r = a.Jvar[m * D] * (vr[0] * vr[0]);
#pragma unroll
            for (int d = 1; d < D; ++d) r = fma(a.Jvar[m * D + d], vr[d] * vr[d], r);
            a.vel_var[m] = r;
        }
    }
    if constexpr (D == 3) {
        if (a.ori_out || a.ori_gap) {
            double B[3][3], q[4], gap;
            tp_jacobian<3>(a.J_ori, m, Rj, B);
            tp_quaternion(B, q, gap);
            if (a.det_ori) a.det_ori[m] = sm_det<3>(B);
            if (a.ori_gap) a.ori_gap[m] = gap;
            if (a.ori_out) {
                const double bw = a.ori[m * 4], bx = a.ori[m * 4 + 1], by = a.ori[m * 4 + 2], bz = a.ori[m * 4 + 3];
                a.ori_out[m * 4] = q[0] * bw - q[1] * bx - q[2] * by - q[3] * bz;
                a.ori_out[m * 4 + 1] = q[0] * bx + q[1] * bw + q[2] * bz - q[3] * by;
                a.ori_out[m * 4 + 2] = q[0] * by - q[1] * bz + q[2] * bw + q[3] * bx;
                a.ori_out[m * 4 + 3] = q[0] * bz + q[1] * by - q[2] * bx + q[3] * bw;
            }
            return;
        }
    }
    if (a.det_ori) {
        double B[D][D];
        tp_jacobian<D>(a.J_ori, m, Rj, B);
        a.det_ori[m] = sm_det<D>(B);
    }
}

void launch_transport_affine(hipStream_t s, int D, const TransportArgs& a) {
    if (a.M <= 0) return;
    const dim3 grid((unsigned)((a.M + 255) / 256));            // M < 2^31: the grid fits
    with_small_dim(D, [&](auto d) { hipLaunchKernelGGL((k_affine<decltype(d)::value>), grid, dim3(256), 0, s, a); });
}

void launch_transport_push(hipStream_t s, int D, const TransportArgs& a) {
    if (a.M <= 0) return;
    const dim3 grid((unsigned)((a.M + 255) / 256));
    with_small_dim(D, [&](auto d) { hipLaunchKernelGGL((k_push_forward<decltype(d)::value>), grid, dim3(256), 0, s, a); });
}

}  // namespace gpt
