// Variational training and prediction of the point-cloud surface SVGP (include/gpt_hip.h: gpt_svgp_surface_train,
// gpt_svgp_surface_elbo_grad, gpt_svgp_surface_predict).  Replaces the reference's plain StocasticVariationalGaussianProcess
// (policy_transportation/models/torch/stocastic_variational_gaussian_process.py:15-105): the whitened ELBO of
// gpt_svgp_train.hip with a length-scale per task, fp64.
//
// Unlike gpt_svgp_train (one workgroup per task), every task's Z x Z work is spread over the whole chip: one optimiser
// step enqueues, per task and in task order, on one stream
//   sf_assemble          K = c k(Z,Z) + eps I padded to NP with identity, W = 0, Kx = c k(Z, X_b) padded to NP x BP
//   launch_factor_inverse  L = chol(K) in place, W = L^-1 (gpt_fit.hip; a non-positive pivot lands in info[t])
//   sf_flag              info[t] -> the call's failure flag; every later glue launch sees it and returns
//   GEMM                 A = W Kx, U = C^T A
//   sf_fwd_stats, sf_fwd_final   mu, |U_k|^2, |A_k|^2, the KL rows; the task's loss, residuals and noise partial
//   GEMM                 CU = C U; sf_abar: Abar = m gmu^T + w (CU - A), d/dm
//   GEMM                 d/dC = w A U^T (block lower triangle), sf_gc_fix adds the KL part
//   GEMM                 B = W^T Abar, P = -1/2 Abar A^T (lower); sf_sym mirrors P into Q = sym(Phi(-Abar A^T))
//   GEMM x 2             Kbar = W^T (Q W) = d loss / d K(Z,Z)
//   sf_partials          one wave per inducing point: Kbar, B against dK/dc, dK/dl_t, dK/dz (fixed-order wave sums)
//   sf_task_final        fixed-order sums of those rows; the task's raw gradients (c_t, noise_t, l_t)
//   sf_adam_task         Adam on the task's own parameters
// and then once per step
//   sf_shared            sums the Z / global-noise partials over the tasks in task order, Adam on them, loss trace.
// Every GEMM has M, N, K multiples of 64 (k_gemm's tiles): the inducing points are padded to NP (a multiple of 512, the
// factor's padding), the minibatch to BP (a multiple of 64); padding is zero, or identity on the diagonal of K and W.
// No floating-point atomics: two runs with the same inputs are bit-identical.  Notation: DESIGN.md "SVGP training".
//
// Device side only: the kernels and the launchers of gpt_svgp_surface.h.  The entry points are in gpt_svgp_surface_host.hip.
#include "gpt_svgp_surface.h"
#include "gpt_svgp_device.h"

using namespace gpt;

namespace {

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline bool failed(const SfArgs& a) { return *a.fail != INT_MAX; }
__device__ inline double* task_theta(const SfArgs& a, int t) { return a.theta + a.SH + (int64_t)t * a.task_stride; }
__device__ inline double* task_grad(const SfArgs& a, int t) { return a.grad + a.SH + (int64_t)t * a.task_stride; }

// K = c k(Z,Z) + eps I (identity in the padding), W = 0, Kx = c k(Z, X_b) (zero padding); x rows: X[idx[b0 + k]], k < b.
__global__ __launch_bounds__(NT) void sf_assemble(SfArgs a, int t, int b0, int b) {
    if (failed(a)) return;
    const double* tt = task_theta(a, t);
    const double c = softplus(tt[0]);
    double il[MAX_D];
    for (int d = 0; d < a.D; ++d) il[d] = 1.0 / softplus(tt[2 + d]);
    const int Zn = a.Zn, NP = a.NP, BP = a.BP, D = a.D;
    const double* Zp = a.theta;
    const int64_t nK = (int64_t)NP * NP, nX = (int64_t)NP * BP;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < nK + nX; e += (int64_t)gridDim.x * NT) {
        if (e < nK) {
            const int i = (int)(e / NP), j = (int)(e - (int64_t)i * NP);
            double v = i == j ? 1.0 : 0.0;
            if (i < Zn && j < Zn) {
                double q = 0.0;
                for (int d = 0; d < D; ++d) { const double u = (Zp[i * D + d] - Zp[j * D + d]) * il[d]; q += u * u; }
                v = c * exp(-0.5 * q) + (i == j ? JITTER : 0.0);
            }
            a.K[e] = v;
            a.W[e] = 0.0;
        } else {
            const int64_t f = e - nK;
            const int i = (int)(f / BP), k = (int)(f - (int64_t)i * BP);
            double v = 0.0;
            if (i < Zn && k < b) {
                const double* x = a.X + (int64_t)a.idx[b0 + k] * D;
                double q = 0.0;
                for (int d = 0; d < D; ++d) { const double u = (Zp[i * D + d] - x[d]) * il[d]; q += u * u; }
                v = c * exp(-0.5 * q);
            }
            a.Kx[f] = v;
        }
    }
}

__global__ void sf_flag(const int* info, int* fail, int code) {
    if (threadIdx.x == 0 && *info != 0) atomicMin(fail, code);
}

// blocks [0, b): column k of A and U -> stat[3k..3k+2] = (mu_k, |U_k|^2, |A_k|^2); blocks [b, b + Zn): row i of the KL:
// klrow[i] = sum_{j <= i} C_ij^2 + m_i^2 - 2 log|C_ii|
__global__ __launch_bounds__(NT) void sf_fwd_stats(SfArgs a, int t, int b) {
    __shared__ double red[NT];
    if (failed(a)) return;
    const int tid = threadIdx.x, NP = a.NP, BP = a.BP, Zn = a.Zn;
    const double* tt = task_theta(a, t);
    const double* mv = tt + SF_HDR;
    const double* Cm = mv + NP;
    if ((int)blockIdx.x < b) {
        const int k = blockIdx.x;
        double mu = 0.0, uu = 0.0, aa = 0.0;
        for (int i = tid; i < Zn; i += NT) {
            const double x = a.A[(int64_t)i * BP + k], u = a.U[(int64_t)i * BP + k];
            mu += x * mv[i]; uu += u * u; aa += x * x;
        }
        mu = block_sum(mu, red); uu = block_sum(uu, red); aa = block_sum(aa, red);
        if (tid == 0) { a.stat[3 * k] = mu; a.stat[3 * k + 1] = uu; a.stat[3 * k + 2] = aa; }
    } else {
        const int i = blockIdx.x - b;
        const double* Ci = Cm + (int64_t)i * NP;
        double s = 0.0;
        for (int j = tid; j <= i; j += NT) s += Ci[j] * Ci[j];
        s = block_sum(s, red);
        if (tid == 0) a.klrow[i] = s + mv[i] * mv[i] - 2.0 * log(fabs(Ci[i]));
    }
}

// one workgroup: the task's loss and noise partial -> sc[0..3] = (loss_t, w, dsig2, sig2); residuals r_k -> rbuf (zero padding)
__global__ __launch_bounds__(NT) void sf_fwd_final(SfArgs a, int t, int b0, int b) {
    __shared__ double red[NT];
    if (failed(a)) return;
    const int tid = threadIdx.x;
    const double* tt = task_theta(a, t);
    const double c = softplus(tt[0]);
    const double sig2 = (NOISE_FLOOR + softplus(tt[1])) + (NOISE_FLOOR + softplus(a.theta[(int64_t)a.Zn * a.D]));
    double pe = 0.0;
    for (int k = tid; k < a.BP; k += NT) {
        double r = 0.0;
        if (k < b) {
            r = a.Y[(int64_t)a.idx[b0 + k] * a.T + t] - a.stat[3 * k];
            pe += r * r + (c + JITTER + a.stat[3 * k + 1] - a.stat[3 * k + 2]);
        }
        a.rbuf[k] = r;
    }
    const double sum_e = block_sum(pe, red);
    double pkl = 0.0;
    for (int i = tid; i < a.Zn; i += NT) pkl += a.klrow[i];
    const double kl = 0.5 * (block_sum(pkl, red) - a.Zn);
    const double w = 1.0 / (b * sig2);
    if (tid == 0) {
        a.sc[0] = 0.5 * (LOG_2PI + log(sig2)) + 0.5 * w * sum_e + kl / a.num_data;
        a.sc[1] = w;
        a.sc[2] = 0.5 / sig2 - 0.5 * w * sum_e / sig2;
        a.sc[3] = sig2;
    }
}

// Abar = m gmu^T + w (C U - A), gmu_k = -w r_k (NP x BP); d loss / d m (rows < Zn, zero padding)
__global__ __launch_bounds__(NT) void sf_abar(SfArgs a, int t, int b) {
    if (failed(a)) return;
    const int NP = a.NP, BP = a.BP;
    const double* mv = task_theta(a, t) + SF_HDR;
    double* gm = task_grad(a, t) + SF_HDR;
    const double w = a.sc[1], invN = 1.0 / a.num_data;
    const int64_t n = (int64_t)NP * BP;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const int i = (int)(e / BP), k = (int)(e - (int64_t)i * BP);
        a.Ab[e] = mv[i] * (-w * a.rbuf[k]) + w * (a.CU[e] - a.A[e]);
        if (e < NP) {
            const int r = (int)e;
            double g = 0.0;
            if (r < a.Zn) {
                double s = 0.0;
                for (int kk = 0; kk < b; ++kk) s += a.A[(int64_t)r * BP + kk] * a.rbuf[kk];
                g = -w * s + mv[r] * invN;
            }
            gm[r] = g;
        }
    }
}

// d loss / d C = w (A U^T) + (C - diag(1 / C_ii)) / N: the GEMM left A U^T on the block lower triangle (w lives on the device
// since sf_fwd_final); zero outside j <= i < Zn
__global__ __launch_bounds__(NT) void sf_gc_fix(SfArgs a, int t) {
    if (failed(a)) return;
    const int NP = a.NP, Zn = a.Zn;
    const double* Cm = task_theta(a, t) + SF_HDR + NP;
    double* gC = task_grad(a, t) + SF_HDR + NP;
    const double invN = 1.0 / a.num_data, w = a.sc[1];
    const int64_t n = (int64_t)NP * NP;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const int i = (int)(e / NP), j = (int)(e - (int64_t)i * NP);
        gC[e] = (i < Zn && j <= i) ? w * gC[e] + (Cm[e] - (i == j ? 1.0 / Cm[e] : 0.0)) * invN : 0.0;
    }
}

// Q: the GEMM wrote the lower triangle; mirror it into the upper one
__global__ __launch_bounds__(NT) void sf_sym(SfArgs a) {
    if (failed(a)) return;
    const int NP = a.NP;
    const int64_t n = (int64_t)NP * NP;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const int i = (int)(e / NP), j = (int)(e - (int64_t)i * NP);
        if (j > i) a.Q[e] = a.Q[(int64_t)j * NP + i];
    }
}

// One wave per inducing point i < Zn (4 per workgroup): with Kbar (in K), B and the kernel recomputed,
//   rowpart[i] = (sum_j Kbar_ij K_ij + sum_k B_ik Kx_ik,  d/dl_d of the same, d = 0..D-1)   (dK/dc = K / c)
//   part_t[2 + i D + d] = d loss / d z_id = -sum_j 2 Kbar_ij K_ij u_ijd / l_d - sum_k B_ik Kx_ik u_ikd / l_d
__global__ __launch_bounds__(NT) void sf_partials(SfArgs a, int t, int b0, int b) {
    if (failed(a)) return;
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.Zn) return;
    const int D = a.D, NP = a.NP, BP = a.BP, Zn = a.Zn;
    const double* tt = task_theta(a, t);
    const double c = softplus(tt[0]);
    double il[MAX_D], zi[MAX_D], pls[MAX_D], gz[MAX_D];
    for (int d = 0; d < D; ++d) { il[d] = 1.0 / softplus(tt[2 + d]); zi[d] = a.theta[i * D + d]; pls[d] = 0.0; gz[d] = 0.0; }
    double pc = 0.0;
    const double* Kb = a.K + (int64_t)i * NP;
    for (int j = lane; j < Zn; j += 64) {
        double q = 0.0;
        for (int d = 0; d < D; ++d) { const double u = (zi[d] - a.theta[j * D + d]) * il[d]; q += u * u; }
        const double f = Kb[j] * (c * exp(-0.5 * q));
        pc += f;
        for (int d = 0; d < D; ++d) {
            const double u = (zi[d] - a.theta[j * D + d]) * il[d];
            pls[d] += f * u * u * il[d];
            gz[d] -= 2.0 * f * u * il[d];
        }
    }
    for (int k = lane; k < b; k += 64) {
        const double f = a.B[(int64_t)i * BP + k] * a.Kx[(int64_t)i * BP + k];
        const double* x = a.X + (int64_t)a.idx[b0 + k] * D;
        pc += f;
        for (int d = 0; d < D; ++d) {
            const double u = (zi[d] - x[d]) * il[d];
            pls[d] += f * u * u * il[d];
            gz[d] -= f * u * il[d];
        }
    }
    pc = wave_sum(pc);
    for (int d = 0; d < D; ++d) { pls[d] = wave_sum(pls[d]); gz[d] = wave_sum(gz[d]); }
    if (lane == 0) {
        double* rp = a.rowpart + (int64_t)i * (1 + D);
        rp[0] = pc;
        double* pt = a.part + (int64_t)t * a.part_stride + 2 + (int64_t)i * D;
        for (int d = 0; d < D; ++d) { rp[1 + d] = pls[d]; pt[d] = gz[d]; }
    }
}

// one workgroup: the task's raw gradients (c_t, noise_t, l_t) and its loss / noise partial for the shared sum
__global__ __launch_bounds__(NT) void sf_task_final(SfArgs a, int t) {
    __shared__ double red[NT];
    if (failed(a)) return;
    const int tid = threadIdx.x, D = a.D;
    const double* tt = task_theta(a, t);
    double* gt = task_grad(a, t);
    const double c = softplus(tt[0]);
    double s = 0.0;
    for (int i = tid; i < a.Zn; i += NT) s += a.rowpart[(int64_t)i * (1 + D)];
    const double dc = block_sum(s, red) / c + 0.5 / a.sc[3];       // + the prior variance term of v_k
    for (int d = 0; d < D; ++d) {
        double p = 0.0;
        for (int i = tid; i < a.Zn; i += NT) p += a.rowpart[(int64_t)i * (1 + D) + 1 + d];
        p = block_sum(p, red);
        if (tid == 0) gt[2 + d] = p * softplus_grad(tt[2 + d]);
    }
    if (tid == 0) {
        gt[0] = dc * softplus_grad(tt[0]);
        gt[1] = a.sc[2] * softplus_grad(tt[1]);
        for (int d = 2 + D; d < SF_HDR; ++d) gt[d] = 0.0;
        double* pt = a.part + (int64_t)t * a.part_stride;
        pt[0] = a.sc[0];
        pt[1] = a.sc[2];
    }
}

__global__ __launch_bounds__(NT) void sf_adam_task(SfArgs a, int t, double lr, double bc1, double bc2s) {
    if (failed(a)) return;
    const int64_t o0 = a.SH + (int64_t)t * a.task_stride;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < a.task_stride; e += (int64_t)gridDim.x * NT) {
        const int64_t o = o0 + e;
        adam(a.theta[o], a.grad[o], a.m1[o], a.m2[o], lr, bc1, bc2s);
    }
}

// shared parameters: fixed-order sums over the tasks, chain rule of the global noise, Adam, loss trace
__global__ __launch_bounds__(NT) void sf_shared(SfArgs a, int step, int apply, double lr, double bc1, double bc2s) {
    if (failed(a)) return;
    const int64_t nz = (int64_t)a.Zn * a.D, T = a.T;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e <= nz; e += (int64_t)gridDim.x * NT) {
        double g = 0.0;
        if (e < nz) {
            for (int t = 0; t < T; ++t) g += a.part[(int64_t)t * a.part_stride + 2 + e];
        } else {
            for (int t = 0; t < T; ++t) g += a.part[(int64_t)t * a.part_stride + 1];
            g *= softplus_grad(a.theta[e]);
        }
        a.grad[e] = g;
        if (apply) adam(a.theta[e], g, a.m1[e], a.m2[e], lr, bc1, bc2s);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += a.part[(int64_t)t * a.part_stride];
        a.loss[step] = s;
    }
}

// ---- prediction ------------------------------------------------------------------------------------------------------
// beta = W^T m (NP), one thread per column j
__global__ __launch_bounds__(NT) void sf_wtm(const double* W, const double* m, int NP, double* beta) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= NP) return;
    double s = 0.0;
    for (int i = j; i < NP; ++i) s += W[(int64_t)i * NP + j] * m[i];
    beta[j] = s;
}

// Kq = c k(Z, x_k) for queries q0 + k (NP x MC, zero padding)
__global__ __launch_bounds__(NT) void sf_kq(const double* Z, const double* Xq, int Zn, int D, int NP, int MC, int64_t q0, int64_t M,
                                            double c, const double* il, double* Kq) {
    const int64_t n = (int64_t)NP * MC;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT) {
        const int i = (int)(e / MC), k = (int)(e - (int64_t)i * MC);
        double v = 0.0;
        if (i < Zn && q0 + k < M) {
            const double* x = Xq + (q0 + k) * D;
            double q = 0.0;
            for (int d = 0; d < D; ++d) { const double u = (Z[i * D + d] - x[d]) * il[d]; q += u * u; }
            v = c * exp(-0.5 * q);
        }
        Kq[e] = v;
    }
}

// one thread per query: mean = a^T m, var = c - |a|^2 + |C^T a|^2, J_d = sum_j beta_j dk(z_j, x)/dx_d
__global__ __launch_bounds__(NT) void sf_pred_cols(const double* Aq, const double* Vq, const double* Kq, const double* m, const double* beta,
                                                   const double* Z, const double* Xq, const double* il, int Zn, int D, int T, int t, int MC,
                                                   int64_t q0, int64_t M, double c, double* mean, double* var, double* J) {
    const int k = blockIdx.x * NT + threadIdx.x;
    if (k >= MC || q0 + k >= M) return;
    const int64_t q = q0 + k;
    const double* x = Xq + q * D;
    double mu = 0.0, aa = 0.0, vv = 0.0, jd[MAX_D];
    for (int d = 0; d < D; ++d) jd[d] = 0.0;
    for (int i = 0; i < Zn; ++i) {
        const double av = Aq[(int64_t)i * MC + k], vq = Vq[(int64_t)i * MC + k];
        mu += av * m[i]; aa += av * av; vv += vq * vq;
        if (J) {
            const double f = beta[i] * Kq[(int64_t)i * MC + k];
            for (int d = 0; d < D; ++d) jd[d] += f * (Z[i * D + d] - x[d]) * il[d] * il[d];
        }
    }
    mean[q * T + t] = mu;
    if (var) var[q * T + t] = c - aa + vv;
    if (J) for (int d = 0; d < D; ++d) J[(q * T + t) * D + d] = jd[d];
}

unsigned grid_for(int64_t n) {
    const int64_t g = (n + NT - 1) / NT;
    return (unsigned)(g < 4096 ? (g > 0 ? g : 1) : 4096);
}

}  // namespace

void gpt::launch_sf_train(hipStream_t s, const SfArgs& a, const int64_t* bb, int64_t n_steps, int apply, double lr) {
    const int T = a.T, Zn = a.Zn, NP = a.NP, BP = a.BP;
    const int64_t NN = (int64_t)NP * NP, NB_ = (int64_t)NP * BP, nz = (int64_t)Zn * a.D, SH = a.SH, task_stride = a.task_stride;
    for (int64_t st = 0; st < n_steps; ++st) {
        const AdamBias bc = adam_bias((double)(st + 1));
        const int b0 = (int)(bb[st] - bb[0]), b = (int)(bb[st + 1] - bb[st]);
        for (int t = 0; t < T; ++t) {
            double* Cp = a.theta + SH + t * task_stride + SF_HDR + NP;
            double* gC = a.grad + SH + t * task_stride + SF_HDR + NP;
            hipLaunchKernelGGL(sf_assemble, dim3(grid_for(NN + NB_)), dim3(NT), 0, s, a, t, b0, b);
            launch_factor_inverse(s, a.K, a.W, NP, a.info + t, a.scr, nullptr, nullptr);
            hipLaunchKernelGGL(sf_flag, dim3(1), dim3(64), 0, s, a.info + t, a.fail, (int)(st * 64 + t));
            launch_dgemm(s, false, false, NP, BP, NP, 1.0, a.W, NP, a.Kx, BP, a.A, BP, false);        // A = W Kx
            launch_dgemm(s, true, false, NP, BP, NP, 1.0, Cp, NP, a.A, BP, a.U, BP, false);           // U = C^T A
            hipLaunchKernelGGL(sf_fwd_stats, dim3(b + Zn), dim3(NT), 0, s, a, t, b);
            hipLaunchKernelGGL(sf_fwd_final, dim3(1), dim3(NT), 0, s, a, t, b0, b);
            launch_dgemm(s, false, false, NP, BP, NP, 1.0, Cp, NP, a.U, BP, a.CU, BP, false);         // CU = C U
            hipLaunchKernelGGL(sf_abar, dim3(grid_for(NB_)), dim3(NT), 0, s, a, t, b);
            launch_dgemm(s, false, true, NP, NP, BP, 1.0, a.A, BP, a.U, BP, gC, NP, true);            // A U^T (lower; w: sf_gc_fix)
            hipLaunchKernelGGL(sf_gc_fix, dim3(grid_for(NN)), dim3(NT), 0, s, a, t);
            launch_dgemm(s, true, false, NP, BP, NP, 1.0, a.W, NP, a.Ab, BP, a.B, BP, false);         // B = W^T Abar
            launch_dgemm(s, false, true, NP, NP, BP, -0.5, a.Ab, BP, a.A, BP, a.Q, NP, true);         // -1/2 Abar A^T (lower)
            hipLaunchKernelGGL(sf_sym, dim3(grid_for(NN)), dim3(NT), 0, s, a);
            launch_dgemm(s, false, false, NP, NP, NP, 1.0, a.Q, NP, a.W, NP, a.M2, NP, false);        // Q W
            launch_dgemm(s, true, false, NP, NP, NP, 1.0, a.W, NP, a.M2, NP, a.K, NP, false);         // Kbar = W^T Q W
            hipLaunchKernelGGL(sf_partials, dim3((Zn + 3) / 4), dim3(NT), 0, s, a, t, b0, b);
            hipLaunchKernelGGL(sf_task_final, dim3(1), dim3(NT), 0, s, a, t);
            if (apply) hipLaunchKernelGGL(sf_adam_task, dim3(grid_for(task_stride)), dim3(NT), 0, s, a, t, lr, bc.bc1, bc.bc2s);
        }
        hipLaunchKernelGGL(sf_shared, dim3(grid_for(nz + 1)), dim3(NT), 0, s, a, (int)st, apply, lr, bc.bc1, bc.bc2s);
    }
}

void gpt::launch_sf_pred_factor(hipStream_t s, const SfPredArgs& p) {
    launch_factor_inverse(s, p.K, p.W, p.NP, p.info, p.scr, nullptr, nullptr);
}

void gpt::launch_sf_pred_chunks(hipStream_t s, const SfPredArgs& p, int t, double c) {
    const int NP = p.NP, MC = p.MC;
    hipLaunchKernelGGL(sf_wtm, dim3((NP + NT - 1) / NT), dim3(NT), 0, s, p.W, p.m, NP, p.beta);
    for (int64_t q0 = 0; q0 < p.M; q0 += MC) {
        hipLaunchKernelGGL(sf_kq, dim3(grid_for((int64_t)NP * MC)), dim3(NT), 0, s, p.Z, p.Xq, p.Zn, p.D, NP, MC, q0, p.M, c, p.il, p.Kq);
        launch_dgemm(s, false, false, NP, MC, NP, 1.0, p.W, NP, p.Kq, MC, p.Aq, MC, false);      // A = W k(Z, x)
        launch_dgemm(s, true, false, NP, MC, NP, 1.0, p.C, NP, p.Aq, MC, p.Vq, MC, false);       // C^T A
        hipLaunchKernelGGL(sf_pred_cols, dim3((MC + NT - 1) / NT), dim3(NT), 0, s, p.Aq, p.Vq, p.Kq, p.m, p.beta, p.Z, p.Xq, p.il, p.Zn,
                           p.D, p.T, t, MC, q0, p.M, c, p.mean, p.var, p.J);
    }
}
