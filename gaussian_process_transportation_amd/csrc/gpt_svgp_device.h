// Device helpers of the two SVGP trainers (gpt_svgp_train.hip, gpt_svgp_surface.hip; device units only): the whitened ELBO's
// softplus, the fixed-order workgroup sum, and Adam with the bias corrections its launchers compute per step.
#pragma once
#include "gpt_svgp_common.h"

namespace gpt {

__device__ inline double softplus(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ inline double softplus_grad(double x) { if (x > 20.0) return 1.0; double z = exp(x); return z / (z + 1.0); }

// Fixed-order sum over the workgroup (every thread returns the total).
__device__ inline double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

// torch.optim.Adam's update of one element (single-tensor path): bc1 = 1 - beta1^k, bc2s = sqrt(1 - beta2^k).
__device__ inline void adam(double& p, double g, double& a, double& b, double lr, double bc1, double bc2s) {
    a = a + (1.0 - BETA1) * (g - a);
    b = b * BETA2 + (1.0 - BETA2) * g * g;
    p = p + (-(lr / bc1)) * (a / (sqrt(b) / bc2s + ADAM_EPS));
}

struct AdamBias { double bc1, bc2s; };       // 1 - beta1^k and sqrt(1 - beta2^k) of optimiser step k = 1, 2, ...
inline AdamBias adam_bias(double k) { return {1.0 - std::pow(BETA1, k), std::sqrt(1.0 - std::pow(BETA2, k))}; }

}  // namespace gpt
