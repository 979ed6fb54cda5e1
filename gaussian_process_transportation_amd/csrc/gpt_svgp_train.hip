// Variational training of the SVGP transport model (include/gpt_hip.h: gpt_svgp_train, gpt_svgp_elbo_grad).
// Replaces the reference's StocasticVariationalGaussianProcess.fit (policy_transportation/models/torch/
// stocastic_variational_gaussian_process_derivatives.py:168-187): Adam on gpytorch's whitened variational ELBO, fp64.
//
// One optimiser step = two launches on one stream, no host synchronisation between steps:
//   svgp_task_step   <<<T, 256>>>  one workgroup per task: forward, the analytic backward, the task's own raw gradients
//                                   and their Adam update; partial gradients of the shared parameters (Z, length-scale,
//                                   global noise) and the task's loss go to part[t]
//   svgp_shared_step <<<1, 256>>>  sums part[0..T-1] in task order, chains the raw length-scale / global noise, Adam
//                                   on the shared parameters, loss trace
// Every reduction runs in a fixed order (no floating-point atomics): two runs with the same inputs are bit-identical.
// Notation and the derivation of the backward: DESIGN.md "SVGP training".
//
// Device side only: the kernels and the launcher of gpt_svgp_train.h.  The entry points are in gpt_svgp_train_host.hip.
#include "gpt_svgp_train.h"
#include "gpt_svgp_device.h"

using namespace gpt;

namespace {

// ---- one task's forward, backward and own-parameter update --------------------------------------------------------
// Workspace (doubles): M0, M1, M2 (Zn x Zn each), Kx, A, U, Ab, B (Zn x bmax each, row stride b), Xb (bmax x D), yb (bmax).
__global__ __launch_bounds__(NT) void svgp_task_step(SvArgs a, int step, int b0, int b, int apply, double lr, double bc1, double bc2s) {
    __shared__ double s_il[MAX_D];           // 1 / length-scale
    __shared__ double s_red[NT];
    __shared__ double s_piv[SV_MAX_Z];       // sqrt of the Cholesky pivots
    __shared__ double s_mu[SV_MAX_B], s_r[SV_MAX_B], s_e[SV_MAX_B];
    if (*a.fail != INT_MAX) return;          // an earlier step stopped on a non-positive pivot
    const int t = blockIdx.x, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int Zn = a.Zn, D = a.D, T = a.T;
    const double* th = a.theta;
    const double* Zp = th + D;
    double* tt = a.theta + a.n_shared + (int64_t)t * a.task_stride;
    double* gt = a.grad + a.n_shared + (int64_t)t * a.task_stride;
    const double* mv = tt + 2;
    const double* Cm = tt + 2 + Zn;
    const double c = softplus(tt[0]);
    const double sig2 = (NOISE_FLOOR + softplus(tt[1])) + (NOISE_FLOOR + softplus(th[D + Zn * D]));
    const int64_t ZZ = (int64_t)Zn * Zn, ZB = (int64_t)Zn * a.bmax;
    double* M0 = a.ws + (int64_t)t * a.ws_stride;
    double* M1 = M0 + ZZ;
    double* M2 = M1 + ZZ;
    double* Kx = M2 + ZZ;
    double* Am = Kx + ZB;
    double* U = Am + ZB;
    double* Ab = U + ZB;
    double* Bm = Ab + ZB;
    double* Xb = Bm + ZB;
    double* yb = Xb + (int64_t)a.bmax * D;

    if (tid < D) s_il[tid] = 1.0 / softplus(th[tid]);
    for (int k = tid; k < b; k += NT) {
        const int row = a.idx[b0 + k];
        for (int d = 0; d < D; ++d) Xb[k * D + d] = a.X[(int64_t)row * D + d];
        yb[k] = a.Y[(int64_t)row * T + t];
    }
    __syncthreads();

    // K(Z,Z) + eps I -> M0 (lower triangle), K(Z,X_b) -> Kx
    for (int64_t e = tid; e < ZZ; e += NT) {
        const int i = (int)(e / Zn), j = (int)(e - (int64_t)i * Zn);
        if (j > i) continue;
        double q = 0.0;
        for (int d = 0; d < D; ++d) { const double u = (Zp[i * D + d] - Zp[j * D + d]) * s_il[d]; q += u * u; }
        M0[e] = c * exp(-0.5 * q) + (i == j ? JITTER : 0.0);
    }
    for (int e = tid; e < Zn * b; e += NT) {
        const int i = e / b, k = e - i * b;
        double q = 0.0;
        for (int d = 0; d < D; ++d) { const double u = (Zp[i * D + d] - Xb[k * D + d]) * s_il[d]; q += u * u; }
        Kx[e] = c * exp(-0.5 * q);
    }
    __syncthreads();

    // Cholesky, right-looking on the unscaled columns (one barrier per column): K_ik -= K_ij K_kj / K_jj, i >= k > j
    for (int j = 0; j < Zn; ++j) {
        const double p = M0[(int64_t)j * Zn + j];
        if (!(p > 0.0)) {                                        // the same value in every thread: a uniform exit
            if (tid == 0) atomicMin(a.fail, step * 64 + t);
            return;
        }
        const double ip = 1.0 / p;
        for (int i = j + 1 + ty; i < Zn; i += 16) {
            const double lij = M0[(int64_t)i * Zn + j] * ip;
            for (int k = j + 1 + tx; k <= i; k += 16) M0[(int64_t)i * Zn + k] -= lij * M0[(int64_t)k * Zn + j];
        }
        __syncthreads();
    }
    for (int j = tid; j < Zn; j += NT) s_piv[j] = sqrt(M0[(int64_t)j * Zn + j]);
    __syncthreads();
    for (int64_t e = tid; e < ZZ; e += NT) {
        const int i = (int)(e / Zn), j = (int)(e - (int64_t)i * Zn);
        M0[e] = j > i ? 0.0 : (i == j ? s_piv[i] : M0[e] / s_piv[j]);
    }
    __syncthreads();

    // W = L^-1 -> M1, one column per thread (forward substitution against e_c)
    for (int cc = tid; cc < Zn; cc += NT) {
        for (int i = 0; i < cc; ++i) M1[(int64_t)i * Zn + cc] = 0.0;
        for (int i = cc; i < Zn; ++i) {
            double s = i == cc ? 1.0 : 0.0;
            const double* Li = M0 + (int64_t)i * Zn;
            for (int j = cc; j < i; ++j) s -= Li[j] * M1[(int64_t)j * Zn + cc];
            M1[(int64_t)i * Zn + cc] = s / Li[i];
        }
    }
    __syncthreads();

    // A = W K(Z,X_b)
    for (int e = tid; e < Zn * b; e += NT) {
        const int i = e / b, k = e - i * b;
        const double* Wi = M1 + (int64_t)i * Zn;
        double s = 0.0;
        for (int j = 0; j <= i; ++j) s += Wi[j] * Kx[j * b + k];
        Am[e] = s;
    }
    __syncthreads();

    // mu = A^T m, U = C^T A
    for (int k = tid; k < b; k += NT) {
        double s = 0.0;
        for (int i = 0; i < Zn; ++i) s += Am[i * b + k] * mv[i];
        s_mu[k] = s;
    }
    for (int e = tid; e < Zn * b; e += NT) {
        const int j = e / b, k = e - j * b;
        double s = 0.0;
        for (int i = j; i < Zn; ++i) s += Cm[(int64_t)i * Zn + j] * Am[i * b + k];
        U[e] = s;
    }
    __syncthreads();

    // v_k = c + eps + |U_k|^2 - |A_k|^2; e_k = (y_k - mu_k)^2 + v_k
    for (int k = tid; k < b; k += NT) {
        double uu = 0.0, aa = 0.0;
        for (int i = 0; i < Zn; ++i) { const double u = U[i * b + k], x = Am[i * b + k]; uu += u * u; aa += x * x; }
        const double r = yb[k] - s_mu[k];
        s_r[k] = r;
        s_e[k] = r * r + (c + JITTER + uu - aa);
    }
    __syncthreads();
    double pe = 0.0;
    for (int k = tid; k < b; k += NT) pe += s_e[k];
    const double sum_e = block_sum(pe, s_red);
    double pkl = 0.0;
    for (int64_t e = tid; e < ZZ; e += NT) {
        const int i = (int)(e / Zn), j = (int)(e - (int64_t)i * Zn);
        if (j <= i) pkl += Cm[e] * Cm[e];
    }
    for (int i = tid; i < Zn; i += NT) pkl += mv[i] * mv[i] - 2.0 * log(fabs(Cm[(int64_t)i * Zn + i]));
    const double kl = 0.5 * (block_sum(pkl, s_red) - Zn);
    const double invN = 1.0 / a.num_data;
    const double w = 1.0 / (b * sig2);
    const double loss_t = 0.5 * (LOG_2PI + log(sig2)) + 0.5 * w * sum_e + kl * invN;
    const double dsig2 = 0.5 / sig2 - 0.5 * w * sum_e / sig2;

    // Abar = m gmu^T + w (C U - A), gmu_k = -w r_k; d/dm, d/dC (own gradients)
    for (int e = tid; e < Zn * b; e += NT) {
        const int i = e / b, k = e - i * b;
        const double* Ci = Cm + (int64_t)i * Zn;
        double s = 0.0;
        for (int j = 0; j <= i; ++j) s += Ci[j] * U[j * b + k];
        Ab[e] = mv[i] * (-w * s_r[k]) + w * (s - Am[e]);
    }
    for (int i = tid; i < Zn; i += NT) {
        double s = 0.0;
        for (int k = 0; k < b; ++k) s += Am[i * b + k] * s_r[k];
        gt[2 + i] = -w * s + mv[i] * invN;
    }
    for (int64_t e = tid; e < ZZ; e += NT) {
        const int i = (int)(e / Zn), j = (int)(e - (int64_t)i * Zn);
        double g = 0.0;
        if (j <= i) {
            double s = 0.0;
            for (int k = 0; k < b; ++k) s += Am[i * b + k] * U[j * b + k];
            g = w * s + (Cm[e] - (i == j ? 1.0 / Cm[e] : 0.0)) * invN;
        }
        gt[2 + Zn + e] = g;
    }
    __syncthreads();

    // B = W^T Abar (= d loss / d K(Z,X_b)); Q = sym(Phi(-Abar A^T)) -> M0 (L is no longer needed)
    for (int e = tid; e < Zn * b; e += NT) {
        const int j = e / b, k = e - j * b;
        double s = 0.0;
        for (int i = j; i < Zn; ++i) s += M1[(int64_t)i * Zn + j] * Ab[i * b + k];
        Bm[e] = s;
    }
    for (int64_t e = tid; e < ZZ; e += NT) {
        const int i = (int)(e / Zn), j = (int)(e - (int64_t)i * Zn);
        const int p = i > j ? i : j, q = i > j ? j : i;
        double s = 0.0;
        for (int k = 0; k < b; ++k) s += Ab[p * b + k] * Am[q * b + k];
        M0[e] = -0.5 * s;
    }
    __syncthreads();
    // Kbar = W^T Q W (= d loss / d K(Z,Z)): M2 = Q W, then M0 = W^T M2
    for (int64_t e = tid; e < ZZ; e += NT) {
        const int i = (int)(e / Zn), l = (int)(e - (int64_t)i * Zn);
        const double* Qi = M0 + (int64_t)i * Zn;
        double s = 0.0;
        for (int j = l; j < Zn; ++j) s += Qi[j] * M1[(int64_t)j * Zn + l];
        M2[e] = s;
    }
    __syncthreads();
    for (int64_t e = tid; e < ZZ; e += NT) {
        const int mm = (int)(e / Zn), l = (int)(e - (int64_t)mm * Zn);
        double s = 0.0;
        for (int i = mm; i < Zn; ++i) s += M1[(int64_t)i * Zn + mm] * M2[(int64_t)i * Zn + l];
        M0[e] = s;
    }
    __syncthreads();

    // shared-parameter partials, one inducing point (row i) per thread:
    //   dK_ij/dc = K_ij / c, dK_ij/dl_d = K_ij diff_d^2 / l_d^3, dK_ij/dz_id = -K_ij diff_d / l_d^2 (both rows of Kbar)
    double* pt = a.part + (int64_t)t * a.part_stride;
    double pc = 0.0, pls[MAX_D];
    for (int d = 0; d < D; ++d) pls[d] = 0.0;
    for (int i = tid; i < Zn; i += NT) {
        double gz[MAX_D];
        for (int d = 0; d < D; ++d) gz[d] = 0.0;
        for (int j = 0; j < Zn; ++j) {
            double q = 0.0;
            for (int d = 0; d < D; ++d) { const double u = (Zp[i * D + d] - Zp[j * D + d]) * s_il[d]; q += u * u; }
            const double kb = M0[(int64_t)i * Zn + j], kk = c * exp(-0.5 * q);
            const double f = kb * kk, f2 = (kb + M0[(int64_t)j * Zn + i]) * kk;
            pc += f;
            for (int d = 0; d < D; ++d) {
                const double u = (Zp[i * D + d] - Zp[j * D + d]) * s_il[d];
                pls[d] += f * u * u * s_il[d];
                gz[d] -= f2 * u * s_il[d];
            }
        }
        for (int k = 0; k < b; ++k) {
            const double f = Bm[i * b + k] * Kx[i * b + k];
            pc += f;
            for (int d = 0; d < D; ++d) {
                const double u = (Zp[i * D + d] - Xb[k * D + d]) * s_il[d];
                pls[d] += f * u * u * s_il[d];
                gz[d] -= f * u * s_il[d];
            }
        }
        for (int d = 0; d < D; ++d) pt[2 + D + i * D + d] = gz[d];
    }
    const double dc = block_sum(pc, s_red) / c + 0.5 / sig2;       // + the prior variance term of v_k
    for (int d = 0; d < D; ++d) {
        const double s = block_sum(pls[d], s_red);
        if (tid == 0) pt[2 + d] = s;
    }
    if (tid == 0) {
        pt[0] = loss_t;
        pt[1] = dsig2;
        gt[0] = dc * softplus_grad(tt[0]);
        gt[1] = dsig2 * softplus_grad(tt[1]);
    }
    __syncthreads();
    if (!apply) return;
    for (int64_t e = tid; e < a.task_stride; e += NT) {
        const int64_t o = a.n_shared + (int64_t)t * a.task_stride + e;
        adam(a.theta[o], a.grad[o], a.m1[o], a.m2[o], lr, bc1, bc2s);
    }
}

// ---- shared parameters: fixed-order sum over the tasks, chain rule, Adam ---------------------------------------------
__global__ __launch_bounds__(NT) void svgp_shared_step(SvArgs a, int step, int apply, double lr, double bc1, double bc2s) {
    if (*a.fail != INT_MAX) return;
    const int D = a.D, Zn = a.Zn, T = a.T;
    for (int64_t e = threadIdx.x; e < a.n_shared; e += NT) {
        double g = 0.0;
        if (e < D) {
            for (int t = 0; t < T; ++t) g += a.part[(int64_t)t * a.part_stride + 2 + e];
            g *= softplus_grad(a.theta[e]);
        } else if (e < D + (int64_t)Zn * D) {
            for (int t = 0; t < T; ++t) g += a.part[(int64_t)t * a.part_stride + 2 + D + (e - D)];
        } else {
            for (int t = 0; t < T; ++t) g += a.part[(int64_t)t * a.part_stride + 1];
            g *= softplus_grad(a.theta[e]);
        }
        a.grad[e] = g;
        if (apply) adam(a.theta[e], g, a.m1[e], a.m2[e], lr, bc1, bc2s);
    }
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += a.part[(int64_t)t * a.part_stride];
        a.loss[step] = s;
    }
}

}  // namespace

void gpt::launch_svgp_steps(hipStream_t s, const SvArgs& a, const int64_t* bb, int64_t n_steps, int apply, double lr) {
    for (int64_t st = 0; st < n_steps; ++st) {
        const AdamBias bc = adam_bias((double)(st + 1));
        const int b0 = (int)(bb[st] - bb[0]), b = (int)(bb[st + 1] - bb[st]);
        hipLaunchKernelGGL(svgp_task_step, dim3(a.T), dim3(NT), 0, s, a, (int)st, b0, b, apply, lr, bc.bc1, bc.bc2s);
        hipLaunchKernelGGL(svgp_shared_step, dim3(1), dim3(NT), 0, s, a, (int)st, apply, lr, bc.bc1, bc.bc2s);
    }
}
