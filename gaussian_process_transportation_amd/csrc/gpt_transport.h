// Epilogue of the transport on the device (gpt_transport.hip): the affine part before the posterior launches and the
// push-forward of positions, velocities and orientations after them (internal header; plain C++, it also compiles under g++
// for the sanitizer builds).  Every pointer is device memory, fp64.  D == O <= 3 (the caller has checked).
#pragma once
#include "gpt_common.h"

namespace gpt {

// Sweeps of the cyclic Jacobi iteration on the symmetric 4 x 4 matrix of the orientation: fixed, no convergence test (a NaN
// leaves after the same six sweeps as everything else).  tests/transport_fused_restatement.py uses the same count.
constexpr int TRANSPORT_JACOBI_SWEEPS = 6;

struct TransportArgs {
    int64_t M;
    double scale;
    const double *R, *c_src, *c_dst;     // gamma(x) = scale R (x - c_src) + c_dst: (D,D) row-major, (D), (D)
    const double* R_jac;                 // (D,D) the Jacobian of gamma as the caller defines it
    const double* pos;                   // (M,D)
    const double* vel;                   // (M,D) or null
    const double* ori;                   // (M,4) w,x,y,z or null
    double* pos_rot;                     // (M,D) gamma(pos): written by k_affine, read by the posterior launches and k_push_forward
    const double* mean;                  // (M,D) posterior mean at pos_rot
    const double* J;                     // (M,D,D) its Jacobian there, or null
    const double* Jvar;                  // (M,D) Jacobian variance there, or null
    const double* J_ori;                 // (M,D,D) the Jacobian at pos (the un-rotated positions), or null
    double* pos_out;                     // (M,D)
    double *vel_out, *vel_var, *det_vel; // (M,D), (M), (M); each may be null
    double *ori_out, *det_ori, *ori_gap; // (M,4), (M), (M); each may be null
};

// pos -> pos_rot
void launch_transport_affine(hipStream_t s, int D, const TransportArgs& a);
// everything else of TransportArgs; arrays that are null are neither read nor written
void launch_transport_push(hipStream_t s, int D, const TransportArgs& a);

}  // namespace gpt
