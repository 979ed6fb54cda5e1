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
#include "gpt_svgp_common.h"

using namespace gpt;

namespace {

constexpr SvgpLimits SF_LIMITS{4096, 32, 1024};
constexpr int SF_HDR = 32;                   // per-task header: [raw_os, raw_noise_t, raw_ls (D), pad]; keeps m and C 16-byte aligned
constexpr int SF_PRED_CHUNK = 1024;          // queries per prediction chunk

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

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

double host_softplus(double x) { return x > 20.0 ? x : std::log1p(std::exp(x)); }

unsigned grid_for(int64_t n) {
    const int64_t g = (n + NT - 1) / NT;
    return (unsigned)(g < 4096 ? (g > 0 ? g : 1) : 4096);
}

int run(int device, const char* who, const SvgpCall& c) {
    const std::string w = who;
    int bmax = 0;
    if (int rc = svgp_validate(w, c, SF_LIMITS, (size_t)c.T * c.D, &bmax)) return rc;
    if (int rc = use_device(w, device)) return rc;
    const int D = c.D, T = c.T, Zn = c.Zn;

    const int NP = (int)round_up(Zn, PAD_N), BP = (int)round_up(bmax, 64);
    const int64_t ZZ = (int64_t)Zn * Zn, NN = (int64_t)NP * NP, NB_ = (int64_t)NP * BP;
    const int64_t nz = (int64_t)Zn * D, SH = round_up(nz + 1, 64), task_stride = SF_HDR + NP + NN, n_theta = SH + T * task_stride;
    std::vector<double> th(n_theta, 0.0);
    for (int64_t e = 0; e < nz; ++e) th[e] = c.Z[e];
    th[nz] = c.raw_noise[T];
    for (int t = 0; t < T; ++t) {
        double* p = th.data() + SH + t * task_stride;
        p[0] = c.raw_os[t];
        p[1] = c.raw_noise[t];
        for (int d = 0; d < D; ++d) p[2 + d] = c.raw_ls[t * D + d];
        for (int i = 0; i < Zn; ++i) p[SF_HDR + i] = c.m[(int64_t)t * Zn + i];
        for (int i = 0; i < Zn; ++i)
            for (int j = 0; j <= i; ++j) p[SF_HDR + NP + (int64_t)i * NP + j] = c.C[t * ZZ + (int64_t)i * Zn + j];   // the strict upper triangle is not a parameter
    }
    std::vector<int> idx32;
    CallBuffers buf;
    CALLCHK(buf.open());
    const hipStream_t s = buf.stream;
    SvgpDevice dev;
    if (int rc = svgp_upload(buf, c, th, &idx32, &dev)) return rc;
    SfArgs a{};
    a.X = dev.X; a.Y = dev.Y; a.idx = dev.idx; a.loss = dev.loss; a.fail = dev.fail;
    a.theta = dev.theta; a.grad = dev.grad; a.m1 = dev.m1; a.m2 = dev.m2;
    a.N = (int)c.N; a.D = D; a.T = T; a.Zn = Zn; a.NP = NP; a.BP = BP; a.num_data = (double)c.num_data;
    a.SH = SH; a.task_stride = task_stride; a.part_stride = 2 + nz;
    CALLCHK(buf.alloc(&a.part, (size_t)T * a.part_stride));
    for (double** p : {&a.K, &a.W, &a.Q, &a.M2}) CALLCHK(buf.alloc(p, (size_t)NN));
    for (double** p : {&a.Kx, &a.A, &a.U, &a.CU, &a.Ab, &a.B}) CALLCHK(buf.alloc(p, (size_t)NB_));
    CALLCHK(buf.alloc(&a.scr, factor_scratch_doubles(NP)));
    CALLCHK(buf.alloc(&a.stat, (size_t)3 * BP));
    CALLCHK(buf.alloc(&a.rbuf, (size_t)BP));
    CALLCHK(buf.alloc(&a.klrow, (size_t)NP));
    CALLCHK(buf.alloc(&a.rowpart, (size_t)NP * (1 + D)));
    CALLCHK(buf.alloc(&a.sc, 8));
    CALLCHK(buf.alloc(&a.info, (size_t)T));
    CALLCHK(hipMemsetAsync(a.grad, 0, (size_t)n_theta * 8, s));
    CALLCHK(hipMemsetAsync(a.info, 0, (size_t)T * sizeof(int), s));

    for (int64_t st = 0; st < c.n_steps; ++st) {
        const AdamBias bc = adam_bias((double)(st + 1));
        const int b0 = (int)(c.bb[st] - c.bb[0]), b = (int)(c.bb[st + 1] - c.bb[st]);
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
            if (c.apply) hipLaunchKernelGGL(sf_adam_task, dim3(grid_for(task_stride)), dim3(NT), 0, s, a, t, c.lr, bc.bc1, bc.bc2s);
        }
        hipLaunchKernelGGL(sf_shared, dim3(grid_for(nz + 1)), dim3(NT), 0, s, a, (int)st, c.apply, c.lr, bc.bc1, bc.bc2s);
    }
    std::vector<double> out(n_theta);
    double* dst[6];
    if (int rc = svgp_read_back(w, s, c, dev, &out, dst)) return rc;
    if (dst[0]) for (int64_t e = 0; e < nz; ++e) dst[0][e] = out[e];
    if (dst[5]) dst[5][T] = out[nz];
    for (int t = 0; t < T; ++t) {
        const double* p = out.data() + SH + t * task_stride;
        if (dst[4]) dst[4][t] = p[0];
        if (dst[5]) dst[5][t] = p[1];
        if (dst[3]) for (int d = 0; d < D; ++d) dst[3][t * D + d] = p[2 + d];
        if (dst[1]) for (int i = 0; i < Zn; ++i) dst[1][(int64_t)t * Zn + i] = p[SF_HDR + i];
        if (dst[2])
            for (int i = 0; i < Zn; ++i)
                for (int j = 0; j < Zn; ++j)
                    if (j <= i || !c.apply) dst[2][t * ZZ + (int64_t)i * Zn + j] = j <= i ? p[SF_HDR + NP + (int64_t)i * NP + j] : 0.0;
    }
    return GPT_OK;
}

}  // namespace

extern "C" int gpt_svgp_surface_train(int device, const double* X, const double* Y, int64_t N, int D, int T, int n_inducing, double* Z,
                                      double* m, double* C, double* raw_lengthscale, double* raw_outputscale, double* raw_noise,
                                      const int64_t* idx, int64_t n_idx, const int64_t* batch_begin, int64_t n_steps, double lr,
                                      double* loss_trace) {
    SvgpCall c{};
    c.X = X; c.Y = Y; c.N = N; c.num_data = N; c.D = D; c.T = T; c.Zn = n_inducing;
    c.Z = Z; c.m = m; c.C = C; c.raw_ls = raw_lengthscale; c.raw_os = raw_outputscale; c.raw_noise = raw_noise;
    c.idx = idx; c.bb = batch_begin; c.n_idx = n_idx; c.n_steps = n_steps; c.lr = lr; c.apply = 1; c.loss_trace = loss_trace;
    return run(device, "gpt_svgp_surface_train", c);
}

extern "C" int gpt_svgp_surface_elbo_grad(int device, const double* Xb, const double* Yb, int64_t b, int64_t num_data, int D, int T,
                                          int n_inducing, const double* Z, const double* m, const double* C, const double* raw_lengthscale,
                                          const double* raw_outputscale, const double* raw_noise, double* loss, double* grad_Z,
                                          double* grad_m, double* grad_C, double* grad_raw_lengthscale, double* grad_raw_outputscale,
                                          double* grad_raw_noise) {
    const double* params[6] = {Z, m, C, raw_lengthscale, raw_outputscale, raw_noise};
    double* grads[6] = {grad_Z, grad_m, grad_C, grad_raw_lengthscale, grad_raw_outputscale, grad_raw_noise};
    return svgp_elbo_grad(run, "gpt_svgp_surface_elbo_grad", SF_LIMITS, device, Xb, Yb, b, num_data, D, T, n_inducing, params, loss, grads);
}

extern "C" int gpt_svgp_surface_predict(int device, const double* Z, const double* m, const double* C, const double* raw_lengthscale,
                                        const double* raw_outputscale, int n_inducing, int D, int T, const double* Xq, int64_t M,
                                        double* mean, double* var, double* J) {
    const std::string w = "gpt_svgp_surface_predict";
    if (!Z || !m || !C || !raw_lengthscale || !raw_outputscale || !Xq || !mean) return fail(GPT_E_ARG, w + ": NULL argument");
    const int Zn = n_inducing;
    if (int rc = svgp_check_model(w, SF_LIMITS, D, T, Zn)) return rc;
    if (M < 1 || M > ((int64_t)1 << 40)) return fail(GPT_E_ARG, w + ": M (queries) must be >= 1");
    const int64_t ZZ = (int64_t)Zn * Zn;
    if (!all_finite(Z, (size_t)Zn * D) || !all_finite(m, (size_t)T * Zn) || !all_finite(C, (size_t)T * ZZ) ||
        !all_finite(raw_lengthscale, (size_t)T * D) || !all_finite(raw_outputscale, T) || !all_finite(Xq, (size_t)M * D))
        return fail(GPT_E_ARG, w + ": non-finite input");
    if (int rc = use_device(w, device)) return rc;
    const int NP = (int)round_up(Zn, PAD_N);
    const int MC = (int)(M < SF_PRED_CHUNK ? round_up(M, 64) : SF_PRED_CHUNK);
    const int64_t NN = (int64_t)NP * NP, NM = (int64_t)NP * MC;

    CallBuffers buf;
    CALLCHK(buf.open());
    const hipStream_t s = buf.stream;
    double *dZ, *dX, *dK, *dW, *dC, *dm, *dbeta, *dKq, *dAq, *dVq, *dscr, *dil, *dmean, *dvar = nullptr, *dJ = nullptr;
    int* dinfo;
    CALLCHK(buf.alloc(&dZ, (size_t)Zn * D));
    CALLCHK(buf.alloc(&dX, (size_t)M * D));
    CALLCHK(buf.alloc(&dK, (size_t)NN));
    CALLCHK(buf.alloc(&dW, (size_t)NN));
    CALLCHK(buf.alloc(&dC, (size_t)NN));
    CALLCHK(buf.alloc(&dm, (size_t)NP));
    CALLCHK(buf.alloc(&dbeta, (size_t)NP));
    CALLCHK(buf.alloc(&dKq, (size_t)NM));
    CALLCHK(buf.alloc(&dAq, (size_t)NM));
    CALLCHK(buf.alloc(&dVq, (size_t)NM));
    CALLCHK(buf.alloc(&dscr, factor_scratch_doubles(NP)));
    CALLCHK(buf.alloc(&dil, (size_t)MAX_D));
    CALLCHK(buf.alloc(&dinfo, 1));
    CALLCHK(buf.alloc(&dmean, (size_t)M * T));
    if (var) CALLCHK(buf.alloc(&dvar, (size_t)M * T));
    if (J) CALLCHK(buf.alloc(&dJ, (size_t)M * T * D));
    CALLCHK(hipMemcpyAsync(dZ, Z, (size_t)Zn * D * 8, hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(dX, Xq, (size_t)M * D * 8, hipMemcpyHostToDevice, s));

    std::vector<double> Kh(NN), Ch(NN), mh(NP), il(MAX_D, 0.0);
    for (int t = 0; t < T; ++t) {
        const double c = host_softplus(raw_outputscale[t]);
        for (int d = 0; d < D; ++d) il[d] = 1.0 / host_softplus(raw_lengthscale[t * D + d]);
        // K = c k(Z,Z) + eps I with identity in the padding (host: O(Z^2 D), once per task and call), C padded, m padded
        for (int64_t e = 0; e < NN; ++e) { Kh[e] = 0.0; Ch[e] = 0.0; }
        for (int i = 0; i < NP; ++i) {
            mh[i] = i < Zn ? m[(int64_t)t * Zn + i] : 0.0;
            if (i >= Zn) { Kh[(int64_t)i * NP + i] = 1.0; continue; }
            for (int j = 0; j <= i; ++j) {
                double q = 0.0;
                for (int d = 0; d < D; ++d) { const double u = (Z[i * D + d] - Z[j * D + d]) * il[d]; q += u * u; }
                const double v = c * std::exp(-0.5 * q) + (i == j ? JITTER : 0.0);
                Kh[(int64_t)i * NP + j] = v;
                Kh[(int64_t)j * NP + i] = v;
                Ch[(int64_t)i * NP + j] = C[t * ZZ + (int64_t)i * Zn + j];
            }
        }
        CALLCHK(hipMemcpyAsync(dK, Kh.data(), (size_t)NN * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemcpyAsync(dC, Ch.data(), (size_t)NN * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemcpyAsync(dm, mh.data(), (size_t)NP * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemcpyAsync(dil, il.data(), (size_t)MAX_D * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemsetAsync(dW, 0, (size_t)NN * 8, s));
        CALLCHK(hipMemsetAsync(dinfo, 0, sizeof(int), s));
        launch_factor_inverse(s, dK, dW, NP, dinfo, dscr, nullptr, nullptr);
        int info = 0;
        CALLCHK(hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, s));
        CALLCHK(hipStreamSynchronize(s));
        if (info != 0)
            return fail(GPT_E_NOT_PD, w + ": non-positive pivot " + std::to_string(info) + " in chol(c_t k(Z,Z) + eps I) of task " + std::to_string(t));
        hipLaunchKernelGGL(sf_wtm, dim3((NP + NT - 1) / NT), dim3(NT), 0, s, dW, dm, NP, dbeta);
        for (int64_t q0 = 0; q0 < M; q0 += MC) {
            hipLaunchKernelGGL(sf_kq, dim3(grid_for(NM)), dim3(NT), 0, s, dZ, dX, Zn, D, NP, MC, q0, M, c, dil, dKq);
            launch_dgemm(s, false, false, NP, MC, NP, 1.0, dW, NP, dKq, MC, dAq, MC, false);      // A = W k(Z, x)
            launch_dgemm(s, true, false, NP, MC, NP, 1.0, dC, NP, dAq, MC, dVq, MC, false);       // C^T A
            hipLaunchKernelGGL(sf_pred_cols, dim3((MC + NT - 1) / NT), dim3(NT), 0, s, dAq, dVq, dKq, dm, dbeta, dZ, dX, dil, Zn, D, T, t, MC,
                               q0, M, c, dmean, dvar, dJ);
        }
        CALLCHK(hipGetLastError());
        CALLCHK(hipStreamSynchronize(s));       // the host images are rewritten for the next task
    }
    CALLCHK(hipMemcpyAsync(mean, dmean, (size_t)M * T * 8, hipMemcpyDeviceToHost, s));
    if (var) CALLCHK(hipMemcpyAsync(var, dvar, (size_t)M * T * 8, hipMemcpyDeviceToHost, s));
    if (J) CALLCHK(hipMemcpyAsync(J, dJ, (size_t)M * T * D * 8, hipMemcpyDeviceToHost, s));
    CALLCHK(hipStreamSynchronize(s));
    return GPT_OK;
}
