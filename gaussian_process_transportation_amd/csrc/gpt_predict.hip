// Prediction kernels for gfx950 (MI355X), templated on the element type (fp64: the exact-GP path of the reference;
// fp32: its SVGP exact-conversion path, which the reference computes in fp32 torch).
//
//  k_mean_jac : posterior mean  mu[m,o] = sum_n k(x_m, X_n) alpha[n,o]   (sklearn/_gpr.py:443-444)
//               and Jacobian    J[m,o,d] = sum_n (X[n,d]-x[m,d])/l_d^2 k(x_m,X_n) alpha[n,o]
//               (reference models/gaussian_process.py:72-90; Matern 3/2 / 5/2: c g(r) in place of k, gpt_exp.h) as one wavefront-reduced contraction:
//               a wave owns QPW queries, its 64 lanes stride the source points, 16 partial sums per
//               query live in registers and are reduced across the wave once at the end.
//
//  k_var      : posterior variance  c + s^2 - |W k*|^2  (sklearn/_gpr.py:454-485 does L \ k*; here
//               W = L^-1 is explicit so the solve becomes a triangular GEMM), the Jacobian variance
//               c g(0)/l_d^2 - |W dk_d|^2 (gaussian_process.py:95-98; g(0) = 1 for RBF, gpt_exp.h) and d var/dx_d = -2 (W dk_d).(W k*)
//               (gaussian_process.py:122-125) on the matrix cores; design notes at the kernel.  With ntask > 1 the
//               A operand is the stack of the tasks' inverse factors (each pre-scaled by its outputscale) and
//               the kernel columns are shared by all tasks: the SVGP exact-conversion model,
//               models/torch/stocastic_variational_gaussian_process_derivatives.py:113-153.
#include "gpt_common.h"
#include "gpt_exp.h"
#include "gpt_plan.h"
#include "gpt_kvar.h"
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace gpt {

// ------------------------------------------------------------------------------------------
// OC = outputs handled by this pass (1..4): only their partial sums are accumulated.
// DW = coordinates carried per point: 3 (source rows of 4: the tuned D <= 3 layout), WIDE_D (rows of 8, D = 4..8) or MAX_D (rows of 16, D = 9..15).
// WJ = false: the mean alone (predict without derivative: configs[1]) — no Jacobian sums, a third fewer vector instructions.
template <typename T, int QPW, int OC, int KT, int DW, bool WJ = true>
__global__ __launch_bounds__(256) void k_mean_jac(KernelParams p, const T* __restrict__ Xs,
                                                  const T* __restrict__ A4, const T* __restrict__ Xq,
                                                  int64_t M, int o_base, T* __restrict__ mean,
                                                  T* __restrict__ J) {
    typedef typename El<T>::v4 v4;
    constexpr int XS = DW == 3 ? 4 : DW;            // elements per source row
    __shared__ double Tt[256];
    if (std::is_same<T, double>::value) {
        Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * QPW;
    if (m0 >= M) return;
    const int D = p.D;
    constexpr T RS2 = (T)0.70710678118654752440;    // coordinates scaled by 1/sqrt(2): k = exp(ln c - |d'|^2)
    // (branch-free: written as `(d < D) ? Xq[..] : 0` every load sat in its own basic block behind its own wait — QPW x DW memory
    // latencies in a row before the first source, as long as the whole contraction at N = 1024; a missing coordinate reads
    // coordinate 0 and is scaled by zero)
    T q[QPW][DW], qsc[DW];
#pragma unroll
    for (int d = 0; d < DW; ++d) qsc[d] = (d < D) ? (T)(p.inv_ls[d] * 0.70710678118654752440) : (T)0;
#pragma unroll
    for (int i = 0; i < QPW; ++i) {
        const int64_t m = (m0 + i < M) ? (m0 + i) : (M - 1);
        const T* qp = Xq + m * D;
#pragma unroll
        for (int d = 0; d < DW; ++d) q[i][d] = qp[d < D ? d : 0];
    }
#pragma unroll
    for (int i = 0; i < QPW; ++i)
#pragma unroll
        for (int d = 0; d < DW; ++d) q[i][d] *= qsc[d];
    T acc[QPW][OC][1 + DW];
#pragma unroll
    for (int i = 0; i < QPW; ++i)
#pragma unroll
        for (int o = 0; o < OC; ++o)
#pragma unroll
            for (int e = 0; e < 1 + DW; ++e) acc[i][o][e] = (T)0;

    const T lnc = (T)p.lnc;
    for (int n = lane; n < p.N; n += 64) {
        T x[DW];
        if constexpr (DW == 3) {
            const v4 xs = *reinterpret_cast<const v4*>(Xs + (size_t)n * 4);
            x[0] = xs[0] * RS2; x[1] = xs[1] * RS2; x[2] = xs[2] * RS2;
        } else {
#pragma unroll
            for (int v = 0; v < DW / 4; ++v) {
                const v4 xs = *reinterpret_cast<const v4*>(Xs + (size_t)n * XS + 4 * v);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[4 * v + e] = xs[e] * RS2;
            }
        }
        const v4 al = *reinterpret_cast<const v4*>(A4 + (size_t)n * 4);
#pragma unroll
        for (int i = 0; i < QPW; ++i) {
            T df[DW];
#pragma unroll
            for (int d = 0; d < DW; ++d) df[d] = x[d] - q[i][d];
            T hh = df[0] * df[0];
#pragma unroll
            for (int d = 1; d < DW; ++d) hh = fma(df[d], df[d], hh);
            if constexpr (WJ && (KT == KT_MATERN32 || KT == KT_MATERN52)) {
                // Matern: the Jacobian sums take c g(r), not c k(r) (gpt_exp.h), both from one exp
                T gv;
                const T kv = kernel_tab_kg<KT>(hh, lnc, Tt, gv);
#pragma unroll
                for (int o = 0; o < OC; ++o) {
                    acc[i][o][0] += kv * al[o];
                    const T tg = gv * al[o];
#pragma unroll
                    for (int d = 0; d < DW; ++d) acc[i][o][1 + d] += tg * df[d];
                }
            } else {
                const T kv = kernel_tab<KT>(hh, lnc, Tt);
#pragma unroll
                for (int o = 0; o < OC; ++o) {
                    const T t = kv * al[o];
                    acc[i][o][0] += t;
                    if (WJ) {
#pragma unroll
                        for (int d = 0; d < DW; ++d) acc[i][o][1 + d] += t * df[d];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < QPW; ++i)
#pragma unroll
        for (int o = 0; o < OC; ++o)
#pragma unroll
            for (int e = 0; e < (WJ ? 1 + DW : 1); ++e) {
                T v = acc[i][o][e];
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
                acc[i][o][e] = v;
            }
    if (lane == 0) {
        const int O = p.O;
        constexpr double S2 = 1.41421356237309504880;     // undo the 1/sqrt(2) on the (X - x) factor
#pragma unroll
        for (int i = 0; i < QPW; ++i) {
            const int64_t m = m0 + i;
            if (m >= M) break;
#pragma unroll
            for (int o = 0; o < OC; ++o) {
                const int oo = o_base + o;
                if (mean) mean[m * O + oo] = acc[i][o][0];
                if (WJ && J) {
#pragma unroll
                    for (int d = 0; d < DW; ++d)
                        if (d < D) J[(m * O + oo) * D + d] = acc[i][o][1 + d] * (T)(p.inv_ls[d] * S2);
                }
            }
        }
    }
}

template <typename T, int DW>
static void launch_mean_jac_t(hipStream_t s, const KernelParams& p, const T* Xs, const T* A4,
                              const T* Xq, int64_t M, T* mean, T* J) {
    constexpr int QPW = DW == 3 ? 2 : 1;                   // queries per wave; 500k queries at N = 8192: 1 -> 9.17 ms, 2 -> 6.19-6.26, 4 -> 6.11 (r3mj)
    // the mean alone (no Jacobian sums: 3 accumulators per query instead of 12): more queries per wave when there are waves enough
    // (M >= 32 768: 8 per SIMD), so that a small model's short source loop (16 iterations at N = 1024) is not dwarfed by the wave's
    // prologue and its cross-lane reductions.  N = 1024, M = 50 000: 0.071 -> 0.064 ms; at M = 10^4 four per wave LOSE 7 - 10 % (r4s38)
    constexpr int QPW_M = DW == 3 ? 4 : 1;
    const bool many = !J && M >= 32768 && QPW_M != QPW;
    const int qpw = many ? QPW_M : QPW;
    const int64_t waves = (M + qpw - 1) / qpw;
    const int64_t blocks = (waves + 3) / 4;
    for (int ob = 0; ob < p.O; ob += 4) {
        const int cnt = (p.O - ob) < 4 ? (p.O - ob) : 4;
        const T* a4 = A4 + (size_t)(ob / 4) * p.NP * 4;
        const dim3 grid((unsigned)blocks);
        auto go = [&](auto kt, auto oc) {
            constexpr int KT = decltype(kt)::value, OC = decltype(oc)::value;
            if (J) hipLaunchKernelGGL((k_mean_jac<T, QPW, OC, KT, DW, true>), grid, dim3(256), 0, s, p, Xs, a4, Xq, M, ob, mean, J);
            else if (many) hipLaunchKernelGGL((k_mean_jac<T, QPW_M, OC, KT, DW, false>), grid, dim3(256), 0, s, p, Xs, a4, Xq, M, ob, mean, J);
            else hipLaunchKernelGGL((k_mean_jac<T, QPW, OC, KT, DW, false>), grid, dim3(256), 0, s, p, Xs, a4, Xq, M, ob, mean, J);
        };
        with_kernel_type(p.ktype, [&](auto kt) {
            switch (cnt) {
                case 1: go(kt, Int<1>{}); break;
                case 2: go(kt, Int<2>{}); break;
                case 3: go(kt, Int<3>{}); break;
                default: go(kt, Int<4>{});
            }
        });
    }
}

void launch_mean_jac(hipStream_t s, const KernelParams& p, const void* Xs, const void* A4,
                     const void* Xq, int64_t M, void* mean, void* J) {
    if (M <= 0 || (!mean && !J)) return;
    with_elem_type(p.dtype, [&](auto t) {
        using T = decltype(t);
        with_coord_width(p.D, [&](auto dw) {
            launch_mean_jac_t<T, decltype(dw)::value>(s, p, (const T*)Xs, (const T*)A4, (const T*)Xq, M, (T*)mean, (T*)J);
        });
    });
}

// A sweep the work split cut along k: add its parts' partial products in part order, then square / reduce as the
// kernel's own epilogue does.  VAR_SPLIT_SLOTS (8) workgroups per cut sweep, one per row group (= wave of k_var), each with a slab
// slot of its own; wave r of the workgroup takes the group's row tile r, same lane -> element map as k_var.  (One workgroup
// per cut sweep until round 4: 14 workgroups x 1.3 MB at configs[1], 18 us at the rate of 14 CUs.)
template <typename T, bool CROSS, int CPQ = 4>
__global__ __launch_bounds__(256) void k_var_combine(VarPlanDev pl, const T* __restrict__ vslab, T* __restrict__ slab) {
    typedef typename El<T>::v4 v4;
    __shared__ T red[2][4][VAR_COLS];
    const VarSplit sp = pl.splits[blockIdx.x / VAR_SPLIT_SLOTS];
    const int grp = blockIdx.x % VAR_SPLIT_SLOTS;
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    v4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4{0, 0, 0, 0};
    for (int v = sp.v_begin; v < sp.v_end; ++v) {
        const v4* src = reinterpret_cast<const v4*>(vslab) + ((size_t)v * 8 + grp) * (16 * 64) + lane;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] += src[(r * 4 + t) * 64];
    }
    T ssq[4] = {0, 0, 0, 0}, crs[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const T v = acc[t][e];
            ssq[t] += v * v;
            if (CROSS) crs[t] += v * __shfl(v, lane & ~(CPQ - 1));
        }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        ssq[t] += __shfl_xor(ssq[t], 16); ssq[t] += __shfl_xor(ssq[t], 32);
        if (CROSS) { crs[t] += __shfl_xor(crs[t], 16); crs[t] += __shfl_xor(crs[t], 32); }
    }
    if (lk == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            red[0][r][16 * t + lc] = ssq[t];
            red[1][r][16 * t + lc] = CROSS ? crs[t] : (T)0;
        }
    }
    __syncthreads();
    if (threadIdx.x < VAR_SLOT) {
        const int which = threadIdx.x >> 6, cl = threadIdx.x & 63;
        T v = (T)0;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) v += red[which][rr][cl];
        slab[((size_t)sp.slot + grp) * VAR_SLOT + threadIdx.x] = v;
    }
}

// Adds the partial sums of a (column block, task) in slot order and turns them into outputs:
// var (M, ntask), Jvar (M, ntask, D), dvar (D, M) (ntask = 1 only).
template <typename T, int NCOMP, bool KSTAR = true>
__global__ __launch_bounds__(64) void k_var_finalize(KernelParams p, VarPlanDev pl, const T* __restrict__ slab, int64_t M,
                                                     const double* __restrict__ hdr, T* __restrict__ var,
                                                     T* __restrict__ Jvar, T* __restrict__ dvar) {
    const int64_t cb = blockIdx.x;
    const int cl = threadIdx.x;
    const int D = p.D, NT = pl.ntask;
    const int64_t col = cb * VAR_COLS + cl;
    const int64_t m = (NCOMP == 1) ? col : ((NCOMP >= 4) ? (col / NCOMP) : (col / D));
    const int cmp = (NCOMP == 1) ? 0 : ((NCOMP >= 4) ? (int)(col & (NCOMP - 1)) + (KSTAR ? 0 : 1) : 1 + (int)(col % D));
    for (int task = 0; task < NT; ++task) {
        T s2 = (T)0, cr = (T)0;
        int s_begin, s_end;
        if (cb < pl.nfull) { s_begin = (int)(cb * NT + task); s_end = s_begin + 1; }      // handled whole by one workgroup
        else {
            const int64_t e = (cb - pl.nfull) * NT + task;
            s_begin = pl.fin[2 * e]; s_end = pl.fin[2 * e + 1];
        }
        for (int s = s_begin; s < s_end; ++s) {
            const T* sl = slab + (size_t)s * VAR_SLOT;
            s2 += sl[cl];
            cr += sl[VAR_COLS + cl];
        }
        if (m >= M) continue;
        const T c = (T)hdr[16 + task];
        if (cmp == 0) {
            if (var) { const T v = c + (T)p.noise - s2; var[m * NT + task] = v < (T)0 ? (T)0 : v; }
        } else {
            const int d = cmp - 1;
            if (d < D) {
                if (Jvar) Jvar[(m * NT + task) * D + d] = c * (T)(kernel_g0(p.ktype) * p.inv_ls[d] * p.inv_ls[d]) - s2;     // c g(0) / l_d^2 - |W dk_d|^2
                if (dvar) dvar[(int64_t)d * M + m] = (T)-2 * cr;
            }
        }
    }
}

template <typename T>
static void launch_var_t(hipStream_t s, const KernelParams& p, const VarWorkspace& ws, const T* Xs, const T* Wf,
                         const T* Xq, int64_t M, int ncomp, T* var, T* Jvar, T* dvar, const double* hdr) {
    const VarPlanDev& pl_all = ws.plan->d;
    T* slab = static_cast<T*>(ws.slab.p);
    T* vslab = static_cast<T*>(ws.vslab.p);
    T* bscr = static_cast<T*>(ws.bscratch.p);
    const dim3 grid((unsigned)pl_all.P), fgrid((unsigned)pl_all.ncb), cgrid((unsigned)pl_all.n_splits * VAR_SPLIT_SLOTS);
    const bool cross = ncomp >= 4 && dvar != nullptr;
    // The persistent workgroups are not synchronised between rounds and drift apart; once they are further apart than a W
    // tile stays in L2 each fetches its own copy of the W stream (mode J+Jvar, 122 rounds in one launch: 155 MB fetched per
    // column block against 68 MB for the same kernel over 31 rounds, L2 hit rate 54 % against 78 %).  A kernel boundary is the
    // one barrier that needs no co-residency: the rounds go out `var_rounds_per_launch` (gpt_plan.h) at a time.  16 per launch: the
    // same run time (269.9-270.5 k/s in one launch, 270.9-271.3 k/s at 8-16), HBM-side bytes 4.99 -> 1.40 TB per 500k queries,
    // L2 hit rate 54 -> 86 % (profiles/r03_kvar_round_drift.txt).
    const int64_t rounds = pl_all.nfull / pl_all.P;
    const int64_t rpl = var_rounds_per_launch(rounds, (int64_t)pl_all.ntask * pl_all.tiles_per_task, 16);
    // fp64 diagonal tiles with the first half of their B image in LDS: for models whose scratch images do not stay in L2 (k_var);
    // GPT_VAR_DIAG_HALF = 0 / 1 forces it off / on (read per call: tests compare both in one process)
    constexpr bool HALF_OK = std::is_same<T, double>::value;          // (fp32 stages the whole image of a diagonal tile in LDS: DIAG_LDS)
    bool diag_half = HALF_OK && pl_all.nbi <= 5;
    if (const char* e = getenv("GPT_VAR_DIAG_HALF")) { if (atoi(e) >= 0) diag_half = HALF_OK && atoi(e) != 0; }
    for (int64_t r0 = 0; r0 == 0 || r0 < rounds; r0 += rpl) {
    VarPlanDev pl = pl_all;
    pl.rnd_begin = r0;
    pl.rnd_end = r0 + rpl < rounds ? r0 + rpl : rounds;
    pl.with_tail = pl.rnd_end >= rounds ? 1 : 0;
    // which instantiation: launch_kvar (gpt_kvar.h).  k* alone: every kernel type, in this unit; derivative columns: RBF in this unit,
    // Matern 3/2 and 5/2 in gpt_predict_matern.hip (Matern 1/2 has none: the API refuses its derivatives before a launch is reached)
    if (ncomp == 1)
        with_kernel_type(p.ktype, [&](auto kt) {
            launch_kvar<T, decltype(kt)::value, false>(ncomp, cross, p.D, diag_half, grid, s, p, pl, Xs, Wf, Xq, M, slab, vslab, bscr);
        });
    else if (p.ktype == KT_MATERN32 || p.ktype == KT_MATERN52)
        launch_var_matern<T>(s, p, pl, ncomp, cross, grid, Xs, Wf, Xq, M, slab, vslab, bscr);
    else
        launch_kvar<T, KT_RBF, true>(ncomp, cross, p.D, diag_half, grid, s, p, pl, Xs, Wf, Xq, M, slab, vslab, bscr);
    }
    const VarPlanDev& pl = pl_all;
    if (pl.n_splits > 0) {
        if (!cross) hipLaunchKernelGGL((k_var_combine<T, false>), cgrid, dim3(256), 0, s, pl, vslab, slab);
        else if (ncomp == 4) hipLaunchKernelGGL((k_var_combine<T, true, 4>), cgrid, dim3(256), 0, s, pl, vslab, slab);
        else if (ncomp == 8) hipLaunchKernelGGL((k_var_combine<T, true, 8>), cgrid, dim3(256), 0, s, pl, vslab, slab);
        else hipLaunchKernelGGL((k_var_combine<T, true, 16>), cgrid, dim3(256), 0, s, pl, vslab, slab);
    }
    switch (ncomp) {
        case VAR_NCOMP_DERIV4: hipLaunchKernelGGL((k_var_finalize<T, 4, false>), fgrid, dim3(64), 0, s, p, pl, slab, M, hdr, var, Jvar, dvar); break;
        case VAR_NCOMP_DERIV8: hipLaunchKernelGGL((k_var_finalize<T, 8, false>), fgrid, dim3(64), 0, s, p, pl, slab, M, hdr, var, Jvar, dvar); break;
        case 1: hipLaunchKernelGGL((k_var_finalize<T, 1>), fgrid, dim3(64), 0, s, p, pl, slab, M, hdr, var, Jvar, dvar); break;
        case 3: hipLaunchKernelGGL((k_var_finalize<T, 3>), fgrid, dim3(64), 0, s, p, pl, slab, M, hdr, var, Jvar, dvar); break;
        case 4: hipLaunchKernelGGL((k_var_finalize<T, 4>), fgrid, dim3(64), 0, s, p, pl, slab, M, hdr, var, Jvar, dvar); break;
        case 8: hipLaunchKernelGGL((k_var_finalize<T, 8>), fgrid, dim3(64), 0, s, p, pl, slab, M, hdr, var, Jvar, dvar); break;
        default: hipLaunchKernelGGL((k_var_finalize<T, 16>), fgrid, dim3(64), 0, s, p, pl, slab, M, hdr, var, Jvar, dvar);
    }
}

void launch_var(hipStream_t s, const KernelParams& p, const VarWorkspace& ws, const void* Xs, const void* Wf,
                const void* Xq, int64_t M, int ncomp, void* var, void* Jvar, void* dvar, const double* hdr) {
    if (M <= 0 || !ws.plan) return;
    with_elem_type(p.dtype, [&](auto t) {
        using T = decltype(t);
        launch_var_t<T>(s, p, ws, (const T*)Xs, (const T*)Wf, (const T*)Xq, M, ncomp, (T*)var, (T*)Jvar, (T*)dvar, hdr);
    });
}

}  // namespace gpt

#ifdef GPT_VAR_TRACE
// trace builds only (make trace): dev_buf holds VT_WGS * 8 * VT_ITEMS * VT_STAMPS int64, or NULL to switch the trace off
extern "C" int gpt_debug_set_var_trace(void* dev_buf) {
    long long* p = static_cast<long long*>(dev_buf);
    return hipMemcpyToSymbol(HIP_SYMBOL(gpt::g_var_trace), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif
