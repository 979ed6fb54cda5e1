// The transported policy at target-space points (gpt_pullback.hip): x = Phi^-1(y), v(y) = J_Phi(x) f(x), with Phi = gamma +
// psi o gamma the fitted transport (psi: the map model, gamma(x) = scale R (x - c_src) + c_dst) and f the mean of a second
// model, the dynamics (internal header; plain C++, it also compiles under g++ for the sanitizer builds).  Every pointer is
// device memory, fp64 unless it says int.  Both models are fp64, single-task, D == O <= 3 with the same D; the map model is
// RBF / Matern 3/2 / Matern 5/2, the dynamics model any of the four kernels (the caller has checked).
#pragma once
#include "gpt_common.h"

namespace gpt {

struct PullbackArgs {
    int64_t M;
    double scale;
    const double *R, *c_src, *c_dst;     // gamma: (D,D) row-major, (D), (D)
    const double* R_jac;                 // (D,D) the Jacobian of gamma as the caller defines it
    const double* Y;                     // (M,D) target-space points
    const double* X0;                    // (M,D) guesses of the preimages (Newton starts at gamma(x0)), or null: start at y
    double rtol;                         // as InverseArgs
    int max_passes;
    double std_offset;                   // s_m = sqrt(var_dyn[m]) - std_offset
    // k_pullback_velocity writes (each may be null except vel and status)
    double* x;                           // (M,D) gamma^-1(z)
    double* z;                           // (M,D) the last accepted point of the Newton iteration on z + psi(z) = y
    double* f;                           // (M,D) mean of the dynamics at x
    double* vel;                         // (M,D) A R_jac f
    double* det;                         // (M) det A
    double* residual;                    // (M) |z + psi(z) - y|
    int* passes;                         // (M)
    int* status;                         // (M) INV_*
    double* A;                           // (M,D,D) I + J_psi(z)
    // k_pullback_variance reads A and f and
    const double* var_dyn;               // (M) raw posterior variance of the dynamics at x, or null
    const double* Jvar;                  // (M,D) Jacobian variance of the map at z, or null
    // and writes (each may be null; the input it consumes is then not read)
    double* vel_var_map;                 // (M)   sum_d Jvar[m,d] (R_jac f)_d^2
    double* vel_var_dyn;                 // (M,D) s_m^2 sum_j (A R_jac)[i,j]^2
};

// Newton, the affine inverse, the dynamics mean and the push-forward: one wave per query, one launch.  pm / pd, Xs_*, A4_*:
// parameters, scaled sources and alpha rows of the map and of the dynamics model.
void launch_pullback_velocity(hipStream_t s, const KernelParams& pm, const double* Xs_map, const double* A4_map, const KernelParams& pd,
                              const double* Xs_dyn, const double* A4_dyn, const PullbackArgs& a);
// vel_var_map and vel_var_dyn, one thread per query
void launch_pullback_variance(hipStream_t s, int D, const PullbackArgs& a);

}  // namespace gpt
