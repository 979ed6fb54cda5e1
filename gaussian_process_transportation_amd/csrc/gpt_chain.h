// The transported policy pulled back through a CHAIN of transports (gpt_chain.hip, gpt_chain_host.hip): Phi = Phi_{K-1} o ... o
// Phi_0, each Phi_k = gamma_k + psi_k o gamma_k a fitted transport as in gpt_pullback.h, and f the mean of one more model, the
// dynamics:  x = Phi^-1(y),  v(y) = J_Phi(x) f(x)  (internal header; plain C++, it also compiles under g++ for the sanitizer
// builds).  Stage 0 is applied first in the forward direction, so it is solved last.  Every pointer is device memory, fp64 unless
// it says int.  All models are fp64, single-task, D == O <= 3 with one D; the stage models are RBF / Matern 3/2 / Matern 5/2, the
// dynamics any of the four kernels (the caller has checked).  Per-stage arrays are stage-major: stage k's rows start at k * M
// rows, so a stage's slice serves as the queries of that stage's variance launch.
#pragma once
#include "gpt_common.h"

namespace gpt {

constexpr int CHAIN_MAX = 4;             // = GPT_CHAIN_MAX of include/gpt_hip.h

// what the wave-level passes read of one model: a cut of KernelParams (D <= 3) and the two arrays of its blob
struct ChainModel {
    int N, ktype;
    double lnc;
    double inv_ls[3];
    const double *Xs, *A4;
};

struct ChainStage {
    ChainModel m;                        // psi_k
    const double *R, *c_src, *c_dst;     // gamma_k: (D,D) row-major, (D), (D)
    const double* R_jac;                 // (D,D) the Jacobian of gamma_k as the caller defines it
    double scale;
};

struct ChainArgs {
    int64_t M;
    int K;                               // 1 .. CHAIN_MAX
    ChainStage st[CHAIN_MAX];
    ChainModel dyn;
    const double* Y;                     // (M,D) target-space points
    const double* X0;                    // (M,D) guesses of the source-space preimages, or null: every stage starts at its own y_k
    double rtol;                         // as InverseArgs
    int max_passes;
    double std_offset;                   // s_m = sqrt(var_dyn[m]) - std_offset
    // k_chain_velocity writes (each may be null except vel and status)
    double* x;                           // (M,D) the preimage under the whole chain, x_0
    double* f;                           // (M,D) mean of the dynamics at x
    double* vel;                         // (M,D) B_{K-1} ... B_0 f,  B_k = A_k R_jac,k
    int* status;                         // (M) INV_* of the first stage in solve order (K-1 first) that is not CONVERGED, else CONVERGED
    double* stage_x;                     // (K,M,D) x_k = gamma_k^-1(z_k), the y of stage k-1
    double* stage_z;                     // (K,M,D) the last accepted point of stage k's Newton iteration
    double* stage_A;                     // (K,M,D,D) I + J_psi_k(z_k)
    int* stage_status;                   // (K,M) INV_*
    int* stage_passes;                   // (K,M)
    double* stage_residual;              // (K,M)
    double* stage_det;                   // (K,M) det A_k
    // k_chain_variance reads stage_A and f and
    const double* var_dyn;               // (M) raw posterior variance of the dynamics at x, or null
    const double* stage_Jvar;            // (K,M,D) Jacobian variance of psi_k at z_k, or null
    // and writes (each may be null; the input it consumes is then not read)
    double* vel_var_map;                 // (M,D) sum_k sigma_k^2 sum_j (B_{K-1} ... B_{k+1})[i,j]^2
    double* vel_var_dyn;                 // (M,D) s_m^2 sum_j (B_{K-1} ... B_0)[i,j]^2
};

// the K inverses, the dynamics mean and the push-forward: one wave per query, one launch
void launch_chain_velocity(hipStream_t s, int D, const ChainArgs& a);
// vel_var_map and vel_var_dyn, one thread per query
void launch_chain_variance(hipStream_t s, int D, const ChainArgs& a);

// arrays of gpt_pullback_chain, in the order of its arguments; ints: status, stage_status, stage_passes
enum { CH_Y = 0, CH_X0, CH_X, CH_VEL, CH_F, CH_STATUS, CH_VAR_DYN, CH_VVAR_MAP, CH_VVAR_DYN, CH_STAGE_X, CH_STAGE_Z, CH_STAGE_A,
       CH_STAGE_JVAR, CH_STAGE_MAP_VAR, CH_STAGE_STATUS, CH_STAGE_PASSES, CH_STAGE_RES, CH_STAGE_DET, CH_COUNT };
constexpr int CH_INPUTS = 2;             // CH_Y, CH_X0 travel to the device, the rest from it
constexpr int CH_FIRST_STAGE = CH_STAGE_X;   // from here on (K,M,...) arrays

}  // namespace gpt
