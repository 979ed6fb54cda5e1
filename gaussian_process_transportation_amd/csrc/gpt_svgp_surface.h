// What the two halves of the surface SVGP unit share (internal header): the limits, the argument structs and the launchers.
// gpt_svgp_surface.hip holds the kernels; gpt_svgp_surface_host.hip holds gpt_svgp_surface_train, _elbo_grad and _predict.
// Plain C++: the sanitizer build compiles it with g++ (host_stub/).
#pragma once
#include "gpt_svgp_common.h"

namespace gpt {

constexpr SvgpLimits SF_LIMITS{4096, 32, 1024};
constexpr int SF_HDR = 32;                   // per-task header: [raw_os, raw_noise_t, raw_ls (D), pad]; keeps m and C 16-byte aligned
constexpr int SF_PRED_CHUNK = 1024;          // queries per prediction chunk

// Device pointers and geometry of one call.
//   theta / grad / m1 / m2: [Z (Zn*D) | raw_noise_global | pad to SH] then per task (task_stride doubles):
//                           [raw_os, raw_noise_t, raw_ls_t (D), pad to SF_HDR | m (NP) | C (NP x NP, lower, zero padding)]
//   part: per task [loss_t, d loss / d noise_t, d loss / d Z (Zn*D)]
struct SfArgs {
    const double* X;      // (N, D)
    const double* Y;      // (N, T)
    const int* idx;       // schedule rows
    double *theta, *grad, *m1, *m2, *part, *loss;
    double *K, *W, *scr, *Kx, *A, *U, *CU, *Ab, *B, *Q, *M2;   // workspace, reused by every task
    double *stat, *rbuf, *klrow, *rowpart, *sc;
    int* info;            // per task: the factor's first non-positive pivot (0: none)
    int* fail;            // INT_MAX, or step * 64 + task of the first non-positive pivot
    int64_t SH, task_stride, part_stride;
    int N, D, T, Zn, NP, BP;
    double num_data;
};

// The n_steps optimiser steps of a training call, every task of a step in task order (the unit's header lists the launches):
// step st takes the rows idx[bb[st] - bb[0] .. bb[st + 1] - bb[0]) of the uploaded schedule (bb: host) and Adam's bias
// corrections of step st + 1.  apply = 0: gradients only.
void launch_sf_train(hipStream_t s, const SfArgs& a, const int64_t* bb, int64_t n_steps, int apply, double lr);

// Device buffers of gpt_svgp_surface_predict.  Per task the host refills K, C, m and il, clears W and info.
struct SfPredArgs {
    const double *Z, *Xq;            // (Zn, D), (M, D)
    double *K, *W;                   // (NP, NP): c_t k(Z,Z) + eps I padded with identity -> its factor; W = L^-1
    const double *C, *m, *il;        // (NP, NP) lower, (NP), 1 / length-scale (MAX_D) of the task
    double *beta, *Kq, *Aq, *Vq;     // (NP); (NP, MC) panels of one chunk of queries
    double* scr;                     // factor_scratch_doubles(NP)
    int* info;                       // the factor's first non-positive pivot (0: none)
    double *mean, *var, *J;          // (M, T), (M, T) or null, (M, T, D) or null
    int Zn, D, T, NP, MC;
    int64_t M;
};
// Factors the task's K in place and inverts the factor into W; a non-positive pivot lands in *info.
void launch_sf_pred_factor(hipStream_t s, const SfPredArgs& p);
// beta = W^T m, then every chunk of MC queries: column t of mean, var and J; c: the task's prior variance.
void launch_sf_pred_chunks(hipStream_t s, const SfPredArgs& p, int t, double c);

}  // namespace gpt
