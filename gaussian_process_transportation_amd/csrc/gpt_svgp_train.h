// What the two halves of the transport SVGP trainer share (internal header): the limits, the kernels' argument struct and the
// launcher.  gpt_svgp_train.hip holds the kernels; gpt_svgp_train_host.hip holds gpt_svgp_train and gpt_svgp_elbo_grad.  Plain
// C++: the sanitizer build compiles it with g++ (host_stub/).
#pragma once
#include "gpt_svgp_common.h"

namespace gpt {

constexpr int SV_MAX_Z = 1024, SV_MAX_B = 1024;              // sizes of svgp_task_step's LDS arrays
constexpr SvgpLimits SV_LIMITS{SV_MAX_Z, 32, SV_MAX_B};

struct SvArgs {
    const double* X;      // (N, D) training inputs
    const double* Y;      // (N, T) training targets
    const int* idx;       // schedule: rows of X / Y
    double* theta;        // parameters: [raw_ls (D) | Z (Zn*D) | raw_noise_global] then per task [raw_os, raw_noise_t, m (Zn), C (Zn*Zn)]
    double* grad;         // gradients, same layout
    double* m1;           // Adam first moments, same layout
    double* m2;           // Adam second moments, same layout
    double* part;         // per task: [loss, d loss / d noise_t, d / d ls (D), d / d Z (Zn*D)]
    double* ws;           // per task workspace
    double* loss;         // per-step loss trace (device)
    int* fail;            // INT_MAX, or step * 64 + task of the first non-positive pivot
    int64_t ws_stride, part_stride, task_stride, n_shared;
    int N, D, T, Zn, bmax;
    double num_data;      // N of the ELBO's KL scaling
};

// The n_steps optimiser steps of a call, two launches each: step st takes the rows idx[bb[st] - bb[0] .. bb[st + 1] - bb[0]) of
// the uploaded schedule (bb: host) and Adam's bias corrections of step st + 1.  apply = 0: gradients only.
void launch_svgp_steps(hipStream_t s, const SvArgs& a, const int64_t* bb, int64_t n_steps, int apply, double lr);

}  // namespace gpt
