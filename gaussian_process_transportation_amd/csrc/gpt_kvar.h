// The variance kernel k_var and its element-type traits, shared by the translation units that instantiate it: gpt_predict.hip
// (everything but the Matern derivative launches) and gpt_predict_matern.hip (those: a unit of their own, so that a parallel
// build compiles the two at the same time).
#pragma once
#include "gpt_common.h"
#include "gpt_dispatch.h"
#include "gpt_exp.h"
#include "gpt_plan.h"
#include <type_traits>

namespace gpt {

// ------------------------------------------------------------------------------------------
// Element-type traits: vector types, the MFMA, and the layout unit of the A stream Wf.
//   fp64: per (k4-step, row group) two d2 per lane (row tiles 0,1 | 2,3): [q 0..2)[lane 0..64)[p 0..2)
//   fp32: per (k4-step, row group) one f4 per lane (row tiles 0..3):       [lane 0..64)[e 0..4)
// 16 B per lane and load either way; the v_mfma_*_16x16x4 A/B lane maps are the same for both types.
// ------------------------------------------------------------------------------------------
template <typename T> struct El;
template <> struct El<double> {
    typedef d4 v4;
    typedef d2 avec;
    static constexpr int A_STEP = 1024, A_GROUP = 128;     // avec per k4-step of a tile / per row group inside it
    static constexpr int SUBS = 4;                         // sub-chunks of 8 k4-steps per LDS chunk: 2 x 32 steps x 2 KiB = 128 KiB
    static constexpr int PF = 2;                           // A fragments are requested this many k4-steps (of 1024 cycles) ahead
    static constexpr bool DIAG_LDS = false;                // the B image of a diagonal tile (256 KiB) does not fit in LDS
    static constexpr bool BATCH_PROLOGUE = false;          // measured in round 1: no gain on the long fp64 sweeps
    struct AF { d2 lo, hi; };
    static __device__ __forceinline__ void lda(AF& a, const avec* __restrict__ p, const int lane) { a.lo = p[lane]; a.hi = p[lane + 64]; }
    static __device__ __forceinline__ void keep(const AF& a, const v4& b) { asm volatile("" :: "v"(a.lo), "v"(a.hi), "v"(b)); }
    static __device__ __forceinline__ void keep1(const v4& b) { asm volatile("" :: "v"(b)); }
    static __device__ __forceinline__ v4 mfma(const double a, const double b, const v4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ void mfma16(v4 (&acc)[4][4], const AF& a, const v4& b) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[0][t] = mfma(a.lo[0], b[t], acc[0][t]);
            acc[1][t] = mfma(a.lo[1], b[t], acc[1][t]);
            acc[2][t] = mfma(a.hi[0], b[t], acc[2][t]);
            acc[3][t] = mfma(a.hi[1], b[t], acc[3][t]);
        }
    }
    // row tiles R0 .. 3 only (the last k-steps of a wave's diagonal 64 x 64 block: zeros above the diagonal)
    template <int R0> static __device__ __forceinline__ void mfma_from(v4 (&acc)[4][4], const AF& a, const v4& b) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (R0 <= 0) acc[0][t] = mfma(a.lo[0], b[t], acc[0][t]);
            if (R0 <= 1) acc[1][t] = mfma(a.lo[1], b[t], acc[1][t]);
            if (R0 <= 2) acc[2][t] = mfma(a.hi[0], b[t], acc[2][t]);
            acc[3][t] = mfma(a.hi[1], b[t], acc[3][t]);
        }
    }
};
template <> struct El<float> {
    typedef f4 v4;
    typedef f4 avec;
    static constexpr int A_STEP = 512, A_GROUP = 64;
    static constexpr int SUBS = 4;                         // 2 x 32 steps x 1 KiB = 64 KiB (64-step chunks measured 4 % slower: profiles/r02_svgp_variants.txt)
    static constexpr int PF = 4;                           // an fp32 MFMA block lasts 512 cycles, less than an L2 round trip under load
    static constexpr bool DIAG_LDS = true;                 // diagonal tiles: B image (128 KiB) staged in LDS
    static constexpr bool BATCH_PROLOGUE = true;           // a reload sweep's first chunk: its four loads in flight together (short fp32 sweeps)
    struct AF { f4 v; };
    static __device__ __forceinline__ void lda(AF& a, const avec* __restrict__ p, const int lane) { a.v = p[lane]; }
    static __device__ __forceinline__ void keep(const AF& a, const v4& b) { asm volatile("" :: "v"(a.v), "v"(b)); }
    static __device__ __forceinline__ void keep1(const v4& b) { asm volatile("" :: "v"(b)); }
    static __device__ __forceinline__ v4 mfma(const float a, const float b, const v4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ void mfma16(v4 (&acc)[4][4], const AF& a, const v4& b) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[0][t] = mfma(a.v[0], b[t], acc[0][t]);
            acc[1][t] = mfma(a.v[1], b[t], acc[1][t]);
            acc[2][t] = mfma(a.v[2], b[t], acc[2][t]);
            acc[3][t] = mfma(a.v[3], b[t], acc[3][t]);
        }
    }
    template <int R0> static __device__ __forceinline__ void mfma_from(v4 (&acc)[4][4], const AF& a, const v4& b) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (R0 <= 0) acc[0][t] = mfma(a.v[0], b[t], acc[0][t]);
            if (R0 <= 1) acc[1][t] = mfma(a.v[1], b[t], acc[1][t]);
            if (R0 <= 2) acc[2][t] = mfma(a.v[2], b[t], acc[2][t]);
            acc[3][t] = mfma(a.v[3], b[t], acc[3][t]);
        }
    }
};

// ------------------------------------------------------------------------------------------
// Variance kernel.
//
// What the hardware does (measured on MI355X, profiles/r01_*):
//   * v_mfma_f64_16x16x4_f64 issues every 64 cycles per SIMD: 77.7 TFLOP/s with 2 waves/SIMD at 2.4 GHz
//     (v_mfma_f32_16x16x4_f32 every 32: 155 TFLOP/s);
//   * every fp64 VALU instruction of a SIMD takes ~4.5 cycles away from its fp64 MFMA stream (the fp64
//     matrix and vector paths share the DP units), so B values must be generated once, not per wave;
//   * a workgroup barrier every 8 k-steps costs ~4 %; once the matrix pipe is >90 % busy the chip lowers
//     its clock (2.38 -> 2.18 GHz), so what is left is energy per MFMA: operands must come from close by
//     (A from L2 with all workgroups walking W in step, B from LDS), not from HBM.
// Design:
//   * a workgroup (512 threads = 8 waves, 2 per SIMD) owns a 64-column block and sweeps the 512-row
//     i-blocks of every task, longest sweep first; wave w accumulates the 64x64 product of its 64-row group (16 MFMA
//     tiles) and folds it into per-column sums when the sweep ends, so V = W K*^T never touches memory
//     (a sweep that the work split cut along k stores its partial product instead: gpt_plan.h);
//   * the B operand of a sweep reaches the waves through a double-buffered LDS image in MFMA lane order,
//     2 x 32 k-steps, one barrier per 32 k-steps.  Wave w fills k-steps w, w+8, w+16,
//     w+24 of the next chunk from the middle of its own MFMA run (the two waves of a SIMD staggered).
//     In a GENERATING sweep the fragments are computed (k* / dk_d columns, one exp each: table-driven in fp64,
//     gpt_exp.h, v_exp_f32 in fp32) and a copy goes to this workgroup's scratch image in HBM/L2
//     ([k-step][lane][4]); the other sweeps of the block reload them from there — so a
//     block pays N exps per column, not N*(N/512+1)/2;
//   * the A operand streams from the fragment-ordered image Wf with 16-byte loads per lane,
//     two k-steps ahead; in the diagonal tile a wave skips the k-steps where its row group is
//     entirely above the diagonal (wave g has 16 (g + 1) of 128), row groups paired (0,7)(1,6)(2,5)(3,4) on
//     the SIMDs.  In every sweep the diagonal tile runs OUTSIDE the lock-step LDS pipeline (every wave on its own; B from the
//     scratch image, to which a generating sweep writes the tile's fragments first — fp64 straight from there, small models with the
//     first half staged in LDS, fp32 with the whole tile's image staged in LDS), so the pairing balances it: 0.56 of a full tile
//     instead of 0.75 (+2.7 %).  And 0.52: the last 16 k-steps of a wave's range are its own lower-triangular 64 x 64 block, whose
//     zero 16 x 16 blocks get no MFMA (not in the instantiations at the register limit: TRI_OK below);
//   * work split: gpt_plan.h (rounds of whole blocks, then an explicit item list cut at quarter tiles — inside diagonal tiles
//     too where a workgroup's share is small).
// Alternatives measured and dropped (profiles/r01_kvar_variant_ab.txt): per-wave B generation (v1, 53 TF),
// 8-step chunks (-3.7 %), barrier-free sweeps with every wave reading B from the scratch image (-3 %: L2
// hit rate 97 % -> 56 %, 3.4 TB/s from beyond L2, clock 2.18 GHz), deeper A prefetch (0 %).
// NCOMP = 1: one column per query (k*).  NCOMP = 4: four columns per query (k*, dk_0, dk_1, dk_2).
// NCOMP = 3: D columns per query (dk_0 .. dk_{D-1}) — the Jacobian variance without the variance.
// DW = 3 is all of the above: D <= 3, source rows of 4 elements, query coordinates in registers.  DW = WIDE_D / MAX_D is the
// wide path for D = 4 .. 8 (rows of 8) / 9 .. 15 (rows of 16): only the generating sweep differs — the block's query coordinates sit in LDS
// (qs[d][query]), distances are coordinate loops — with NCOMP = 1, or NCOMP = 8 / 16: k*, dk_0 .. dk_{D-1} and zero
// columns up to 8 (D <= 7) or 16 per query, so that a query's columns stay inside one 16-column MFMA tile.  KSTAR = false
// (wide path, NCOMP = 4 for D = 4 and 8 for D = 8): the Jacobian variance alone, dk_0 .. dk_{D-1} without the k* column —
// half the columns of the fused layout at exactly those two dimensions.
// ------------------------------------------------------------------------------------------
// Timing-only ablation builds (results are wrong unless 0), every live number:
//   -DGPT_ABL=1 no per-chunk barrier, 2 no A-operand loads in the lock-step loop, 3 diagonal tile skipped, 4 no B fill (LDS image
//   left as is), 5 no MFMAs, 6 every wave 72 steps in a diagonal tile (the work of a SIMD's pair split evenly)
//   (make ablate, tools/gpu_ablate.sh, profiles/r01_final_ablation.txt);
//   7 generating sweep without the exp (the squared distance itself is stored), 8 no copy of the generated fragments to the scratch
//   image, 9 no fold of the accumulators into the column sums (small models: tools/small_n_probe.py);
//   12 the diagonal tile without its A stream (past its first 8 k-steps), 13 the diagonal tile without its B reads.
#ifndef GPT_ABL
#define GPT_ABL 0
#endif
// -DGPT_VAR_TRACE (make trace): shader-clock stamps (s_memtime) of every wave of two workgroups at the phase boundaries of
// their first VT_ITEMS items, written to the buffer set through gpt_debug_set_var_trace.
#ifdef GPT_VAR_TRACE
constexpr int VT_STAMPS = 16, VT_ITEMS = 24, VT_WGS = 2;
__device__ long long* g_var_trace = nullptr;
// (inline asm with AMDGPU constraints has to sit in a __device__ function: in the body of a __global__ template the host
// pass rejects the constraint, silently drops the kernel's host stub and the library no longer loads)
static __device__ __forceinline__ long long vt_clock() {
    long long t_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory");
    return t_;
}
// the chip-wide 100 MHz counter (s_memtime counts per XCD: workgroups on different XCDs cannot be compared with it)
static __device__ __forceinline__ long long vt_realtime() {
    long long t_;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory");
    return t_;
}
#define GPT_VT(i) do { if (vt_base && lane == 0 && it < VT_ITEMS) vt_base[(size_t)it * VT_STAMPS + (i)] = vt_clock(); } while (0)
#else
#define GPT_VT(i) do { } while (0)
#endif
constexpr int VAR_SUB = 8;          // k4-steps per sub-chunk (= waves per workgroup: wave w fills step w of each)
// chunk double buffer (fp64: 2 x 32 steps x 2 KiB = 128 KiB; fp32: 64 KiB) or, fp32, the B image of a diagonal tile (128 steps x 1 KiB)
template <typename T> constexpr size_t var_lds_bytes() {
    constexpr size_t chunks = (size_t)2 * VAR_SUB * El<T>::SUBS * 64 * 4 * sizeof(T), image = (size_t)WT_K4 * 64 * 4 * sizeof(T);
    return (El<T>::DIAG_LDS && image > chunks) ? image : chunks;
}

// fp64 Matern kernels with derivative columns: they sit at the register limit (their generating code keeps more alive: r, the
// column kind).  Without the diagonal triangle, with the 2-deep ring of the diagonal tile and with late source loads (wide rows)
// no spill code is left in a hot loop (tools/check_isa_spills.py; with the RBF kernels' settings 2 - 8 reloads sat in them).
// (A namespace-scope constant: as a local constexpr read inside k_var's lambdas it changed the code hipcc emits for RBF kernels.
// The mechanism, for whoever edits the kernel: its lambdas capture by reference, in the order of first use — and inside the generic
// ones a name in an expression that depends on the lambda's parameter is captured even where a constant would do.  Which of k_var's
// locals a closure holds, and in what order, reaches the instruction order and the register numbers of the code hipcc emits,
// although the closures themselves are optimised away.  A helper that names a local in a new place — even inside a branch that is
// compiled out — therefore changes kernels it never runs in; tools/device_isa_diff.py against the parent commit shows which.)
template <typename T, int NCOMP, int KT>
constexpr bool kvar_tight = NCOMP != 1 && KT != KT_RBF && std::is_same<T, double>::value;

template <typename T, int NCOMP, bool CROSS, int KT, int DW = 3, bool KSTAR = true, bool HALF = false>
__global__ __launch_bounds__(512, 2) void k_var(KernelParams p, VarPlanDev pl, const T* __restrict__ Xs,
                                                const T* __restrict__ Wf, const T* __restrict__ Xq,
                                                int64_t M, T* __restrict__ slab, T* __restrict__ vslab, T* __restrict__ bscratch) {
    typedef typename El<T>::v4 v4;
    typedef typename El<T>::avec avec;
    typedef typename El<T>::AF AF;
    constexpr size_t A_STEP = El<T>::A_STEP;
    constexpr int VAR_SUBS = El<T>::SUBS;               // sub-chunks per LDS chunk
    constexpr int VAR_CH = VAR_SUB * VAR_SUBS;          // k4-steps per LDS chunk, one barrier each (32 fp64 / 64 fp32; divides 128)
    extern __shared__ __attribute__((aligned(16))) unsigned char Bs_raw[];       // [buffer][k4-step][lane][column tile]
    T* const Bs_dyn = reinterpret_cast<T*>(Bs_raw);
    constexpr bool WIDE = DW != 3;
    constexpr int XS = WIDE ? DW : 4;                   // elements per source row
    constexpr int CPQ = NCOMP >= 4 ? NCOMP : 1;         // columns per query when they sit side by side (a power of two)
    static_assert(!WIDE || (DW == 8 && (NCOMP == 1 || NCOMP == 8 || NCOMP == 16 || (!KSTAR && NCOMP == 4))) || (DW == 16 && KSTAR && (NCOMP == 1 || NCOMP == 16)),
                  "wide path: rows of 8, NCOMP 1 / 8 / 16 (4 / 8 without k*); rows of 16, NCOMP 1 / 16");
    static_assert(WIDE || NCOMP == 1 || NCOMP == 3 || NCOMP == 4, "D <= 3: NCOMP 1 / 3 / 4");
    static_assert(KSTAR || (WIDE && !CROSS && (NCOMP == 4 || NCOMP == 8)), "no k* column: wide path, Jacobian variance alone");
    __shared__ T red[2][8][VAR_COLS];
    __shared__ double Tt[256];
    __shared__ T qs[WIDE ? DW : 1][VAR_COLS];           // wide path: scaled coordinates of this block's queries, [d][query]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lc = lane & 15, lk = lane >> 4;
    const int g = (w < 4) ? w : (11 - w);     // row group of this wave: 0,1,2,3,7,6,5,4
    const int D = p.D;
    auto Bs = [&](const int buf, const int step) -> T* { return Bs_dyn + ((size_t)(buf * VAR_CH + step) * 64 + lane) * 4; };
    if (std::is_same<T, double>::value && threadIdx.x < 256) Tt[threadIdx.x] = g_exp2_table[threadIdx.x];
#ifdef GPT_VAR_TRACE
    long long* vt_base = nullptr;
    if (g_var_trace && (blockIdx.x == 0 || blockIdx.x == 37))
        vt_base = g_var_trace + ((size_t)(blockIdx.x == 0 ? 0 : 1) * 8 + w) * VT_ITEMS * VT_STAMPS;
    // begin / end time (100 MHz, chip-wide) of every workgroup (wave 0), behind the phase stamps: [VT_WGS * 8 * VT_ITEMS * VT_STAMPS + 2 * blockIdx.x]
    long long* const vt_wg = (g_var_trace && threadIdx.x == 0 && blockIdx.x < 1024) ? g_var_trace + (size_t)VT_WGS * 8 * VT_ITEMS * VT_STAMPS + 2 * blockIdx.x : nullptr;
    if (vt_wg) vt_wg[0] = vt_realtime();
#endif

    constexpr T RS2 = (T)0.70710678118654752440;    // coordinates are pre-scaled by 1/sqrt(2): t = ln c - |d'|^2
    // NCOMP=4: column = 4 query + comp, comp = lc & 3 in every tile: b = kv * (cbv + sum_d cd[d] * d'_d).
    // NCOMP=3 (Jacobian variance alone, no k* column): column = D query + d, D columns per query; for D = 3 the d of a
    // lane's column changes from tile to tile and from block to block (16 = 64 = 1 mod 3), selected in `produce`.
    const int comp = (CPQ > 1) ? (lc & (CPQ - 1)) + (KSTAR ? 0 : 1) : 0;      // 0: the k* column, 1 + d: dk_d
    const T cbv = (comp == 0) ? (T)1 : (T)0;
    T cd[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) cd[d] = (!WIDE && comp == d + 1 && d < D) ? (T)(p.inv_ls[d] * 1.41421356237309504880) : (T)0;
    // wide path: a derivative column needs one coordinate beyond the distance, its own: dimension own_d, factor sc_own
    // (zero in the k* column and in the zero columns)
    const int own_d = (WIDE && comp >= 1 && comp <= D) ? comp - 1 : 0;
    T sc_own = (T)0;
    if (WIDE) {
#pragma unroll
        for (int d = 0; d < DW; ++d) if (comp == d + 1 && d < D) sc_own = (T)(p.inv_ls[d] * 1.41421356237309504880);
    }
    // Matern kernels: a derivative column is c g(r) u_d, not c k(r) u_d (gpt_exp.h kernel_tab_col: both from one exp); the k* column
    // keeps c k.  RBF (g = k) and the k*-only launches generate with kernel_tab, as before.
    static_assert(NCOMP == 1 || KT != KT_MATERN12, "Matern 1/2 has no derivative columns");
    constexpr bool GCOL = NCOMP != 1 && KT != KT_RBF;
    const bool dcol = NCOMP == 3 || comp != 0;
    const T lnc = (T)p.lnc;
    const int nbi = pl.nbi;
    // A stream: element (step S, group g, ...) — uniform base + per-lane 32-bit offset (scalar-base addressing: no
    // 64-bit VALU address arithmetic, and no VALU writes into registers that loads are still in flight to)
    const avec* const wuni = reinterpret_cast<const avec*>(Wf) + (size_t)g * El<T>::A_GROUP;
    // this workgroup's B image: k-step s, lane l at s*64 + l (v4 units)
    v4* const buni = reinterpret_cast<v4*>(bscratch) + (size_t)blockIdx.x * ((size_t)p.NP * 16);

    const int per_block = pl.ntask * nbi;                       // sweeps of a whole block
    const int64_t n_implicit = (pl.rnd_end - pl.rnd_begin) * per_block;     // this launch's rounds
    const int it_begin = pl.item_begin[blockIdx.x], it_end = pl.item_begin[blockIdx.x + 1];

    T ssq[4] = {0, 0, 0, 0}, crs[4] = {0, 0, 0, 0};
    for (int64_t it = 0;; ++it) {
        // ---- next item: derived (rounds of whole blocks, in step with every other workgroup) or listed (tail)
        int64_t cb; int task, ib, k_lo, k_hi, flags, slot, vslot;
        if (it < n_implicit) {
            const int64_t rl = it / per_block;
            const int r = (int)(it - rl * per_block);
            const int64_t rnd = pl.rnd_begin + rl;
            task = r / nbi;
            ib = nbi - 1 - (r - task * nbi);
            cb = rnd * pl.P + blockIdx.x;
            k_lo = 0; k_hi = VAR_KQ * (ib + 1);
            flags = (r == 0 ? (VI_FIRST | VI_GEN) : 0) | (ib == nbi - 1 ? VI_ZERO : 0);
            slot = (ib == 0) ? (int)(cb * pl.ntask + task) : -1;
            vslot = -1;
        } else {
            const int64_t idx = it_begin + (it - n_implicit);
            if (!pl.with_tail || idx >= it_end) break;
            const VarItem item = pl.items[idx];
            cb = item.cb; task = item.task; ib = item.ib; k_lo = item.k_lo; k_hi = item.k_hi;
            flags = item.flags; slot = item.slot; vslot = item.vslot;
        }
        GPT_VT(0);
        if (flags & VI_FIRST) {
            __syncthreads();                               // LDS (Bs, red, Tt) free / ready
            // The scratch image changes owner: block n's fragments overwrite block n - 1's.  Writers and readers of a workgroup's
            // image are the waves of THAT workgroup, i.e. of one CU, and its vector L1 is coherent among them (a store through the
            // L1 updates or drops the line it hits; AMDGPU memory model, non-tgsplit mode: "no special action is required for
            // coherence between wavefronts in the same work-group") — so workgroup scope is the scope that is needed: ordering, no
            // cache invalidation.  (An AGENT-scope acquire, buffer_inv sc1, cost 20 000 - 35 000 clocks at the
            // opening of every block, 3 % of the kernel at N = 1024: profiles/r04_small_n.txt.)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        } else if (flags & VI_GEN) {
            __syncthreads();                               // nobody may still be reading the part of the image rewritten now
        }
        if (WIDE && (flags & VI_FIRST)) {
            // the block's queries (64 for NCOMP = 1, 64 / NCOMP otherwise), coordinate w (and w + 8 in rows of 16) by wave w, scaled as the sources are
            constexpr int NQ = VAR_COLS / (CPQ > 1 ? CPQ : 1);
            const int64_t m = cb * NQ + lane;
            const int64_t mm = (m < M) ? m : (M - 1);
#pragma unroll
            for (int c0 = 0; c0 < DW; c0 += 8) {
                const int cw = c0 + w;
                double il = 0.0;
#pragma unroll
                for (int d = 0; d < DW; ++d) if (d == cw) il = p.inv_ls[d];
                if (lane < NQ) qs[cw][lane] = (cw < D) ? Xq[mm * D + cw] * (T)(il * 0.70710678118654752440) : (T)0;
            }
            __syncthreads();
        }
        if (flags & VI_ZERO) {
#pragma unroll
            for (int t = 0; t < 4; ++t) { ssq[t] = (T)0; crs[t] = (T)0; }
        }
        GPT_VT(1);
        const int base3 = (NCOMP == 3) ? (int)((cb * VAR_COLS + lc) % D) : 0;
        const T sc3[3] = {(T)(p.inv_ls[0] * 1.41421356237309504880), (T)(p.inv_ls[1] * 1.41421356237309504880),
                          (T)(p.inv_ls[2] * 1.41421356237309504880)};

        // One sweep.  GEN = true: B fragments are generated and a copy is kept in the scratch image; GEN = false: they
        // are reloaded from it.  Two instantiations, so that the query coordinates and exp temporaries of the generating
        // sweep do not occupy registers in the others.
        auto sweep = [&](auto gen_tag) {
            constexpr bool GEN = decltype(gen_tag)::value;
            // this lane's four columns (one per MFMA column tile): scaled query coordinates
            GPT_VT(11);
            T q[4][3];
            if (GEN && !WIDE) {
                // twelve loads, no branch between them (a missing coordinate reads coordinate 0 and is scaled by zero): written as
                // `(d < D) ? Xq[..] : 0` each load sat in its own basic block behind its own s_waitcnt vmcnt(0) — twelve memory
                // latencies in a row at the opening of every generating sweep (r04_small_n.txt; a prefetch of the next block's
                // coordinates into LDS by the waves that finish the last diagonal tile early was also built: with the loads batched it
                // saved 1 500 clocks per block and cost the 3-column kernel spill code in its hot loop — removed)
                T raw[4][3], qsc[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) qsc[d] = (d < D) ? (T)(p.inv_ls[d] * 0.70710678118654752440) : (T)0;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int64_t col = cb * VAR_COLS + 16 * t + lc;
                    const int64_t m = (NCOMP == 1) ? col : ((NCOMP == 4) ? (col >> 2) : (col / D));
                    const int64_t mm = (m < M) ? m : (M - 1);
                    const T* qp = Xq + mm * D;
#pragma unroll
                    for (int d = 0; d < 3; ++d) raw[t][d] = qp[d < D ? d : 0];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int d = 0; d < 3; ++d) q[t][d] = raw[t][d] * qsc[d];
            }
#ifdef GPT_VAR_TRACE
            if (GEN) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }      // (trace builds: the query coordinates have arrived)
            GPT_VT(9);
#endif
            // rows of 16 (and the wide kernels with cross terms): the source's coordinates are read where they are used (produce_to), four
            // at a time — carried across the MFMA steps like the narrower rows' they are 16 - 32 more registers than the fp64 kernel has, and
            // it spilled inside its loops
            constexpr bool LATE_X = GEN && WIDE && (DW == 16 || CROSS || kvar_tight<T, NCOMP, KT>);
            T gx[LATE_X ? 1 : DW];                         // coordinates of the source this wave generates next
            T gx_own = (T)0;                               // (wide) and the one a derivative column multiplies by
            v4 bl;                                         // or the fragments it reloads next
            auto load_x_to = [&](const T* xp, auto& ox, T& oown) {
                if constexpr (LATE_X) {
                    (void)xp; (void)ox; (void)oown;
                } else if constexpr (WIDE) {
#pragma unroll
                    for (int v = 0; v < DW / 4; ++v) {
                        const v4 xv = *reinterpret_cast<const v4*>(xp + 4 * v);
#pragma unroll
                        for (int e = 0; e < 4; ++e) ox[4 * v + e] = xv[e];
                    }
                    if (NCOMP != 1) oown = xp[own_d];
                } else {
                    ox[0] = xp[0]; ox[1] = xp[1]; ox[2] = xp[2];
                }
            };
            auto load_x = [&](const T* xp) { load_x_to(xp, gx, gx_own); };
            // The exp of a generating sweep: the kernel value of a column from its squared distance hh (scaled: t = ln c - hh).  GCOL:
            // Matern with derivative columns, where a derivative column (dcol) takes c g(r) and the k* column c k(r), both from one exp
            // (gpt_exp.h).  One column, or a lane's four with the exps stage by stage (their latencies overlap).  Where the four are taken
            // one after the other, that loop stands at the call: inside a helper it changed the instruction order of four fp32 wide
            // Matern 5/2 kernels.  -DGPT_ABL=7 stores the squared distance itself.
            auto kernel_value = [&](const T hh) -> T {
                if (GPT_ABL == 7) return hh;
                if constexpr (GCOL) return kernel_tab_col<KT>(hh, lnc, Tt, dcol);
                else return kernel_tab<KT>(hh, lnc, Tt);
            };
            auto kernel_values_staged = [&](T (&hh)[4], T (&kv)[4]) {
                if (GPT_ABL == 7) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) kv[t] = hh[t];
                } else if constexpr (GCOL) kernel_tab4_col<KT>(hh, lnc, Tt, dcol, kv);
                else kernel_tab4<KT>(hh, lnc, Tt, kv);
            };
            // B fragments of k-step k4 -> LDS chunk buffer `buf` (to_lds) and, when generated, the scratch image
            // staged: the four exps of a lane stage by stage (gpt_exp.h kernel_tab4: their latencies overlap — the openings of a
            // sweep, where no MFMA hides them); not staged: one after the other, as few live registers as possible (inside the
            // MFMA loop, where the staged form spills)
            auto produce_to = [&](auto lds_tag, auto staged_tag, const int buf, const int k4, const bool to_scr = true, const bool lds_on = true) {
                constexpr bool to_lds = decltype(lds_tag)::value;
                constexpr bool staged = decltype(staged_tag)::value;
                T* dstl = Bs(buf, k4 % VAR_CH);
                if constexpr (LATE_X) {
                    const T* xp = Xs + (size_t)(k4 * 4 + lk) * XS;
                    const T xo = (NCOMP != 1) ? xp[own_d] * RS2 : (T)0;
                    v4 b;
                    T hh[4] = {(T)0, (T)0, (T)0, (T)0}, kv[4];
#pragma unroll
                    for (int v = 0; v < DW / 4; ++v) {
                        const v4 xv = *reinterpret_cast<const v4*>(xp + 4 * v);
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int qi = (16 * t + lc) / (CPQ > 1 ? CPQ : 1);      // this column's query within the block
#pragma unroll
                            for (int e = 0; e < 4; ++e) { const T df = fma(xv[e], RS2, -qs[4 * v + e][qi]); hh[t] = fma(df, df, hh[t]); }
                        }
                    }
                    if constexpr (staged) kernel_values_staged(hh, kv);
                    else {
#pragma unroll
                        for (int t = 0; t < 4; ++t) kv[t] = kernel_value(hh[t]);
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int qi = (16 * t + lc) / (CPQ > 1 ? CPQ : 1);
                        b[t] = (NCOMP == 1) ? kv[t] : kv[t] * (cbv + sc_own * (xo - qs[own_d][qi]));
                    }
                    if (to_lds && lds_on) *reinterpret_cast<v4*>(dstl) = b;
                    if (to_scr) (buni + (size_t)k4 * 64)[lane] = b;
                } else if constexpr (GEN && WIDE) {
                    T x[DW];
#pragma unroll
                    for (int d = 0; d < DW; ++d) x[d] = gx[d] * RS2;
                    const T xo = gx_own * RS2;
                    v4 b;
                    T hh[4], kv[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int qi = (16 * t + lc) / (CPQ > 1 ? CPQ : 1);      // this column's query within the block
                        T df = x[0] - qs[0][qi];
                        hh[t] = df * df;
#pragma unroll
                        for (int d = 1; d < DW; ++d) { df = x[d] - qs[d][qi]; hh[t] = fma(df, df, hh[t]); }
                    }
                    if constexpr (staged) kernel_values_staged(hh, kv);
                    else {
#pragma unroll
                        for (int t = 0; t < 4; ++t) kv[t] = kernel_value(hh[t]);
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int qi = (16 * t + lc) / (CPQ > 1 ? CPQ : 1);
                        b[t] = (NCOMP == 1) ? kv[t] : kv[t] * (cbv + sc_own * (xo - qs[own_d][qi]));
                    }
                    if (to_lds && lds_on) *reinterpret_cast<v4*>(dstl) = b;
                    if (to_scr) (buni + (size_t)k4 * 64)[lane] = b;
                } else if (GEN) {
                    const T x0 = gx[0] * RS2, x1 = gx[1] * RS2, x2 = gx[2] * RS2;
                    v4 b;
                    auto column = [&](const int t, const T kv, const T d0, const T d1, const T d2_) -> T {
                        if (NCOMP == 3) {
                            int dsel = base3 + ((D == 3) ? t : 0);            // (64 cb + 16 t + lc) mod D, base3 = (64 cb + lc) mod D
                            dsel = (dsel >= D) ? dsel - D : dsel;
                            const T e = (dsel == 0) ? d0 * sc3[0] : ((dsel == 1) ? d1 * sc3[1] : d2_ * sc3[2]);
                            return kv * e;
                        }
                        return (NCOMP == 1) ? kv : kv * (cbv + cd[0] * d0 + cd[1] * d1 + cd[2] * d2_);
                    };
                    if constexpr (staged) {
                        T d0[4], d1[4], d2_[4], hh[4], kv[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            d0[t] = x0 - q[t][0]; d1[t] = x1 - q[t][1]; d2_[t] = x2 - q[t][2];
                            hh[t] = d0[t] * d0[t];
                            hh[t] = fma(d1[t], d1[t], hh[t]);
                            hh[t] = fma(d2_[t], d2_[t], hh[t]);
                        }
                        kernel_values_staged(hh, kv);
#pragma unroll
                        for (int t = 0; t < 4; ++t) b[t] = column(t, kv[t], d0[t], d1[t], d2_[t]);
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const T d0 = x0 - q[t][0], d1 = x1 - q[t][1], d2_ = x2 - q[t][2];
                            T hh = d0 * d0;
                            hh = fma(d1, d1, hh);
                            hh = fma(d2_, d2_, hh);
                            b[t] = column(t, kernel_value(hh), d0, d1, d2_);
                        }
                    }
                    if (to_lds && lds_on) *reinterpret_cast<v4*>(dstl) = b;
                    if (GPT_ABL != 8 && to_scr) (buni + (size_t)k4 * 64)[lane] = b;
                } else {
                    *reinterpret_cast<v4*>(dstl) = bl;
                }
            };
            auto produce = [&](const int buf, const int k4) { produce_to(std::true_type{}, std::false_type{}, buf, k4); };
            // GEN: `cnt` k-steps k4_0 + j * stride generated with their source loads in flight together (load -> wait -> exp ->
            // store one at a time cost 9.5 k cycles per k-step at the opening of a sweep: profiles/r04_small_n.txt)
            auto generate_batch = [&](auto lds_tag, auto cnt_tag, const int buf, const int k4_0, const int stride, const bool to_scr = true,
                                      const bool lds_on = true) {
                constexpr int cnt = decltype(cnt_tag)::value;
                T bx[cnt][LATE_X ? 1 : DW], bo[cnt];
#pragma unroll
                for (int j = 0; j < cnt; ++j) { bo[j] = (T)0; load_x_to(Xs + (size_t)((k4_0 + j * stride) * 4 + lk) * XS, bx[j], bo[j]); }
#pragma unroll
                for (int j = 0; j < cnt; ++j) {
#pragma unroll
                    for (int d = 0; d < (LATE_X ? 1 : DW); ++d) gx[d] = bx[j][d];
                    gx_own = bo[j];
                    produce_to(lds_tag, std::true_type{}, buf, k4_0 + j * stride, to_scr, lds_on);
                }
            };

            const size_t S_ib = (size_t)task * pl.tiles_per_task * WT_K4 + (size_t)64 * ib * (ib + 1);   // stream index of k4-step 0 of this i-block
            static_assert(VAR_CH == VAR_Q_COST && WT_K4 == VAR_KQ * VAR_CH, "an item's k range counts LDS chunks (quarter tiles)");
            // the item's part of the diagonal tile: k4-steps [d_lo, d_hi) of it — the whole tile (0, 128) everywhere except in the lists
            // of small launches, where the plan may cut it at quarters (gpt_plan.h: cut_diag)
            const bool has_diag = k_hi > VAR_KQ * ib;
            const int d_lo = (k_lo > VAR_KQ * ib ? k_lo - VAR_KQ * ib : 0) * VAR_CH, d_hi = (k_hi - VAR_KQ * ib) * VAR_CH;
            const int K0 = k_lo * VAR_CH;                                      // first k4-step of this item
            // The diagonal tile (where wave g only has 16 (g + 1) steps of work) runs OUT of the lock-step LDS pipeline: see
            // below.  A generating sweep first puts that tile's fragments into the scratch image (inside the lock-step part the
            // tile costs 0.75 of a full one instead of 0.56).
            // (GEN stands in this expression although both kinds of sweep do the same: without a name that depends on the lambda's
            // parameter, `sweep` no longer captures VAR_CH, and hipcc then allocates the registers of the fp32 k* kernels differently —
            // cf. kvar_tight above)
            const int lock_end = ((GEN ? !has_diag : !has_diag) ? k_hi : VAR_KQ * ib) * VAR_CH;
            const int ch0 = K0 / VAR_CH, ch1 = lock_end / VAR_CH;              // lock-step chunks [ch0, ch1)
            // fp64, small models (HALF: its own instantiation of the kernel, so that the N = 8192 kernel keeps its code and registers):
            // the first 64 k-steps of a diagonal tile's B image go through LDS — see the tile below
            constexpr bool half = HALF && !El<T>::DIAG_LDS;
            if (GEN && has_diag && GPT_ABL != 3 && !half) {
                // 128 k-steps (of a whole tile), 16 per wave (w, w + 8, ...), VALU only; complete and visible before the barrier below
                const int kd0 = ib * WT_K4;
#pragma unroll 1
                for (int j = d_lo / VAR_SUB; j < d_hi / VAR_SUB; ++j)
                    generate_batch(std::false_type{}, std::integral_constant<int, 1>{}, 0, kd0 + w + VAR_SUB * j, VAR_SUB);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            GPT_VT(10);
            if (ch1 > ch0) {                                  // first chunk: wave w fills steps w, w+8, w+16, w+24
                if (GEN) {
                    // ONE copy of the generating code, run VAR_SUBS times: the opening of a sweep is straight-line code that runs once
                    // per block, i.e. from a cold instruction cache — its time followed its LENGTH, not its arithmetic (four k-steps
                    // unrolled and batched: 40 000 clocks; twenty: 60 000; serial or staged exps: no difference — r04_small_n.txt)
#pragma unroll 1
                    for (int j = 0; j < VAR_SUBS; ++j)
                        generate_batch(std::true_type{}, std::integral_constant<int, 1>{}, ch0 & 1, K0 + j * VAR_SUB + w, VAR_SUB);
                } else if (El<T>::BATCH_PROLOGUE) {
                    // the four reloads in flight together instead of load -> wait -> write four times (short fp32 sweeps:
                    // 12 per block at configs[4], each opening with this latency)
                    v4 pre[VAR_SUBS];
#pragma unroll
                    for (int j = 0; j < VAR_SUBS; ++j) pre[j] = (buni + (size_t)(K0 + j * VAR_SUB + w) * 64)[lane];
#pragma unroll
                    for (int j = 0; j < VAR_SUBS; ++j) *reinterpret_cast<v4*>(Bs(ch0 & 1, (K0 + j * VAR_SUB + w) % VAR_CH)) = pre[j];
                } else {
                    // (fp64: measured in round 1, no gain from batching on its long sweeps)
#pragma unroll
                    for (int j = 0; j < VAR_SUBS; ++j) {
                        bl = (buni + (size_t)(K0 + j * VAR_SUB + w) * 64)[lane];
                        produce(ch0 & 1, K0 + j * VAR_SUB + w);
                    }
                }
            }
            GPT_VT(2);
            constexpr int PF = El<T>::PF;                  // divides VAR_SUB, so step s of every sub-chunk uses ring slot s % PF
            AF a_ring[PF];                                 // A fragments of the next PF steps
#pragma unroll
            for (int i = 0; i < PF; ++i)                   // the first 16 steps of an item are active for every group
                El<T>::lda(a_ring[i], wuni + (S_ib + K0 + i) * A_STEP, lane);
            __syncthreads();
            GPT_VT(3);
            v4 acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[r][t] = v4{0, 0, 0, 0};
            const int my_limit = ib * WT_K4 + 16 * (g + 1);     // first k4-step of the i-block with nothing left for this group
            // Sources of the fills inside the loop, as loop-carried per-lane pointers (k-step K0 + VAR_CH + w first, then
            // VAR_SUB further each time): an address recomputed from the k-step lands in whatever registers are free —
            // the previous fill's destination registers — and that write-after-load made hipcc drain vmcnt to 0 (and with
            // it the A fragments in flight) at the top of every sub-chunk.
            const v4* bsrc = buni + (size_t)(K0 + VAR_CH + w) * 64 + lane;
            const T* xsrc = Xs + (size_t)((K0 + VAR_CH + w) * 4 + lk) * XS;
            auto fetch_next = [&]() {
                if (GEN) {
                    load_x(xsrc);
                    xsrc += VAR_SUB * 4 * XS;
                } else {
                    bl = bsrc[0];
                    bsrc += VAR_SUB * 64;
                }
            };
            // the chunk body exists twice — with and without the fill of the following chunk — so that "is there a next
            // chunk" is no branch (and no join in front of the first MFMAs of a sub-chunk) inside it
            auto chunk = [&](auto more_tag, const int ch) {
                constexpr bool more = decltype(more_tag)::value;
                const int cur = ch & 1;
                v4 b_nxt = *reinterpret_cast<const v4*>(Bs(cur, 0));    // B fragments are read one k-step ahead
                for (int sub = 0; sub < VAR_SUBS; ++sub) {
                    const int k0 = ch * VAR_CH + sub * VAR_SUB;                 // first k-step of this sub-chunk
                    const int kn = (ch + 1) * VAR_CH + sub * VAR_SUB + w;       // the k-step this wave fills meanwhile
                    if (more) fetch_next();
                    const bool active = (k0 < my_limit) && !(GPT_ABL == 3 && k0 >= ib * WT_K4);   // my_limit is a multiple of 16: all or nothing
                    auto step = [&](const int s) {
                        const int k4 = k0 + s;
                        const AF a = a_ring[s % PF];
                        const v4 b = b_nxt;
                        const int kl = my_limit - 1;
                        const size_t Sn = S_ib + ((k4 + PF < my_limit) ? (k4 + PF) : kl);
                        if (GPT_ABL != 2) El<T>::lda(a_ring[s % PF], wuni + Sn * A_STEP, lane);
                        const int sn = sub * VAR_SUB + s + 1;
                        if (sn < VAR_CH) b_nxt = *reinterpret_cast<const v4*>(Bs(cur, sn));
                        if (GPT_ABL == 5) { El<T>::keep(a, b); return; }
                        El<T>::mfma16(acc, a, b);
                    };
                    // The fill of the next chunk sits INSIDE the active / idle paths, not behind their join: vmcnt counts in
                    // issue order, and behind a join hipcc has to wait for vmcnt(0) — which also waits for the A fragments
                    // the steps just before have requested (a full L2 round trip per sub-chunk); inside the straight-line
                    // path it waits for the fill's own loads only.
                    if (active) {
                        step(0); step(1);
                        if (more && w < 4 && GPT_ABL != 4) produce(cur ^ 1, kn);
                        step(2); step(3); step(4); step(5);
                        if (more && w >= 4 && GPT_ABL != 4) produce(cur ^ 1, kn);
                        step(6); step(7);
                    } else {
                        if (more && GPT_ABL != 4) produce(cur ^ 1, kn);
                        if (sub + 1 < VAR_SUBS) b_nxt = *reinterpret_cast<const v4*>(Bs(cur, (sub + 1) * VAR_SUB));
                    }
                }
                if (GPT_ABL != 1) __syncthreads();
            };
            for (int ch = ch0; ch + 1 < ch1; ++ch) chunk(std::true_type{}, ch);
            if (ch1 > ch0) chunk(std::false_type{}, ch1 - 1);
            GPT_VT(4);
            if (has_diag && GPT_ABL != 3) {
                // Diagonal tile, barrier-free: every wave runs its own 16 (g + 1) k-steps on its own.  No
                // lock-step, so the waves with g and 7 - g that share a SIMD add up to the same work on every SIMD: the tile
                // costs 0.56 of a full one instead of the 0.75 it costs inside the lock-step pipeline.
                const int kd0 = ib * WT_K4;                              // first k-step of the diagonal tile
                const int lim_g = (GPT_ABL == 6) ? 72 : 16 * (g + 1);    // multiple of 16 (ablation 6: every wave the average, 72: what an even split inside a SIMD would cost)
                const int limit = lim_g < d_hi ? lim_g : d_hi;           // this wave's steps: [d_lo, limit), none if limit <= d_lo
                const avec* ap = wuni + (S_ib + kd0) * A_STEP;
                const v4* bp = buni + (size_t)kd0 * 64;
                auto ldA = [&](AF& a, const int k) {
                    const int kk = k < limit ? k : limit - 1;            // clamped: redundant, in bounds
                    if (GPT_ABL == 12 && k >= d_lo + 8) return;          // (timing-only ablation: the tile without its A stream)
                    El<T>::lda(a, ap + (size_t)kk * A_STEP, lane);
                };
                // The last 16 k-steps of a wave's range are its own 64 x 64 diagonal block of the factor (when the item's range reaches
                // that far): W is lower triangular, so row tile r of the group has nothing but zeros from the block's k-step 4 (r + 1)
                // on, and those MFMAs — 24 of the block's 64 tile-steps, 8 % of the whole tile — are not issued.  Adding 0 x b changes
                // nothing, so results are the same to the bit.  body(first row tile with work, k4) runs RR steps from k4.
                // (Not in the instantiations that sit at the register limit — cross terms, the fp64 3-column kernel, wide Matern, fp64
                // Matern derivatives: the peeled steps cost them a spilled pointer inside the ring loop, tools/check_isa_spills.py.)
                constexpr bool TRI_OK = !CROSS && !(std::is_same<T, double>::value && NCOMP == 3) && !(WIDE && KT != KT_RBF) && !kvar_tight<T, NCOMP, KT>;
                const bool tri = TRI_OK && limit == lim_g && limit > d_lo && GPT_ABL != 6;
                auto tri_loop = [&](auto rtag, const int k_begin, const int k_end, const bool tri_end, auto&& body) {
                    constexpr int RR = decltype(rtag)::value;
                    static_assert(RR == 2 || RR == 4, "ring depth of the diagonal tile");
                    const int k_main = tri_end ? k_end - 12 : k_end;
                    for (int k4 = k_begin; k4 < k_main; k4 += RR) body(std::integral_constant<int, 0>{}, k4);
                    if (tri_end) {
                        if constexpr (RR == 4) {
                            body(std::integral_constant<int, 1>{}, k_end - 12); body(std::integral_constant<int, 2>{}, k_end - 8);
                            body(std::integral_constant<int, 3>{}, k_end - 4);
                        } else {
                            body(std::integral_constant<int, 1>{}, k_end - 12); body(std::integral_constant<int, 1>{}, k_end - 10);
                            body(std::integral_constant<int, 2>{}, k_end - 8); body(std::integral_constant<int, 2>{}, k_end - 6);
                            body(std::integral_constant<int, 3>{}, k_end - 4); body(std::integral_constant<int, 3>{}, k_end - 2);
                        }
                    }
                };
                if constexpr (El<T>::DIAG_LDS) {
                    // fp32: B through LDS.  With each wave re-reading its 16 (g + 1) steps of the B image from L2 / Infinity Cache
                    // (as the fp64 path below does) the tile cost 0.75 of a full one after all: 576 KiB per tile and workgroup
                    // in half the time an fp64 tile gives (profiles/r02_svgp_variants.txt).  The whole image of the tile — 128
                    // k-steps x 1 KiB — fits in LDS now that the chunk buffers are free (the last chunk's barrier has passed):
                    // the 8 waves copy it ONCE, 16 k-steps each, then run barrier-free with B from LDS.
                    v4* const img = reinterpret_cast<v4*>(Bs_dyn);       // [k-step 0..128)[lane]
                    constexpr int DP = El<T>::PF;
                    AF a[DP];
#pragma unroll
                    for (int i = 0; i < DP; ++i) ldA(a[i], d_lo + i);
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        if (d_lo >= 64 * (half + 1) || d_hi <= 64 * half) continue;      // (workgroup-uniform: not a k-step of this item)
                        v4 r[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) r[j] = (bp + (size_t)(w + 8 * (8 * half + j)) * 64)[lane];
#pragma unroll
                        for (int j = 0; j < 8; ++j) img[(w + 8 * (8 * half + j)) * 64 + lane] = r[j];
                    }
                    __syncthreads();
                    GPT_VT(12);
                    v4 b_nxt = img[d_lo * 64 + lane];
                    tri_loop(std::integral_constant<int, DP>{}, d_lo, limit > d_lo ? limit : d_lo, tri, [&](auto jtag, const int k4) {
#pragma unroll
                        for (int i = 0; i < DP; ++i) {
                            const v4 b = b_nxt;
                            const int kn = (k4 + i + 1 < limit) ? (k4 + i + 1) : (limit - 1);
                            if (GPT_ABL != 13) b_nxt = img[kn * 64 + lane];          // (13: timing-only, the tile without its B reads)
                            El<T>::template mfma_from<decltype(jtag)::value>(acc, a[i], b);
                            ldA(a[i], k4 + i + DP);
                        }
                    });
                    GPT_VT(14);
                    __syncthreads();                                     // the image is free again (next sweep's first fill)
                } else {
                    // fp64: A from Wf and B straight from the scratch image, both one MFMA block (1024 cycles) ahead; program
                    // order pinned with sched_barrier so hipcc keeps the loads away from their first use.  (Staging the first
                    // 64 k-steps of the image in LDS, as far as 128 KiB go, was 1.1 % slower — two more barriers per tile — for 4 %
                    // fewer fetched bytes: profiles/r02_kvar_diag_image_fp64.txt.)
                    auto ldB = [&](v4& b, const int k) {
                        const int kk = k < limit ? k : limit - 1;
                        if (GPT_ABL == 13 && k >= d_lo + 8) return;
                        b = (bp + (size_t)kk * 64)[lane];
                    };
                    // operand ring depth: 4, or 2 = the loop of rounds 1-3 for the 3-column kernel and the register-tight ones, whose generating
                    // side keeps more state alive: with the deeper ring hipcc reloads a spilled pointer inside the loop, and that reload's
                    // wait drains the ring
                    constexpr int R = (NCOMP == 3 || kvar_tight<T, NCOMP, KT>) ? 2 : 4;
                    if constexpr (half) {
                        // Small models (N <= 2560): the B images of an XCD's 32 workgroups (0.5 MB each at N = 1024) do not stay in its
                        // 4 MB of L2, a diagonal tile read straight from the scratch image is 576 wave-steps x 2 KiB from beyond L2, the
                        // wave that is alone on its SIMD runs at the latency of those reads, and the 256 KB a generating sweep writes
                        // for its own diagonal tile leave 256 workgroups at the same moment (60 000 clocks per opening:
                        // profiles/r04_small_n.txt).  Here the first 64 k-steps of the tile's image — all that waves 0..3 need, half of
                        // what waves 4..7 need — sit in LDS (the chunk buffers are free: the last lock-step barrier has passed): a
                        // generating sweep produces them there (and in the scratch image only when a later sweep will reload them), a
                        // reload sweep copies them from the scratch image ONCE, 8 k-steps per wave; steps 64.. still come from the
                        // scratch image, R blocks ahead.  Two barriers per tile (at N = 8192, where the image is L2-resident, that was
                        // a loss of 1.1 %: r02_kvar_diag_image_fp64.txt — hence by size).
                        v4* const img = reinterpret_cast<v4*>(Bs_dyn);    // [k-step 0..64)[lane] = Bs(buf = k / 32, k % 32)
                        if constexpr (GEN) {
                            const bool priv = it < n_implicit && pl.ntask == 1;      // the top sweep's own tile: nobody reloads these k-steps
#pragma unroll 1
                            for (int j = d_lo / VAR_SUB; j < d_hi / VAR_SUB; ++j) {      // k-steps kd0 + w + 8 j: below 64 -> LDS (+ scratch unless private), the rest -> scratch
                                const int k = kd0 + w + VAR_SUB * j;
                                const bool low = j < 8;
                                generate_batch(std::true_type{}, std::integral_constant<int, 1>{}, low ? (k - kd0) / VAR_CH : 0, k, VAR_SUB, !(priv && low), low);
                            }
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        } else {
#pragma unroll
                            for (int hh = 0; hh < 2; ++hh) {
                                if (d_lo >= 32 * (hh + 1) || d_hi <= 32 * hh) continue;      // (workgroup-uniform)
                                v4 r[4];
#pragma unroll
                                for (int j = 0; j < 4; ++j) r[j] = (bp + (size_t)(w + 8 * (4 * hh + j)) * 64)[lane];
#pragma unroll
                                for (int j = 0; j < 4; ++j) img[(w + 8 * (4 * hh + j)) * 64 + lane] = r[j];
                            }
                        }
                        __syncthreads();
                        GPT_VT(12);
                        AF a[R];
                        v4 b[R];
#pragma unroll
                        for (int i = 0; i < R; ++i) ldA(a[i], d_lo + i);
                        const int l1 = limit < 64 ? limit : 64;
                        const int p2 = d_lo > 64 ? d_lo : 64;             // first step that comes from the scratch image
                        v4 b_nxt = img[(d_lo < 64 ? d_lo : 63) * 64 + lane];
                        tri_loop(std::integral_constant<int, R>{}, d_lo, l1 > d_lo ? l1 : d_lo, tri && limit <= 64, [&](auto jtag, const int k4) {
#pragma unroll
                            for (int i = 0; i < R; ++i) {
                                const v4 bb = b_nxt;
                                const int kn = (k4 + i + 1 < l1) ? (k4 + i + 1) : (l1 - 1);
                                b_nxt = img[kn * 64 + lane];
                                __builtin_amdgcn_sched_barrier(0);
                                El<T>::template mfma_from<decltype(jtag)::value>(acc, a[i], bb);
                                __builtin_amdgcn_sched_barrier(0);
                                ldA(a[i], k4 + i + R);
                            }
                        });
                        GPT_VT(13);
                        if (limit > p2) {
#pragma unroll
                            for (int i = 0; i < R; ++i) ldB(b[i], p2 + i);
                        }
                        tri_loop(std::integral_constant<int, R>{}, p2, limit > p2 ? limit : p2, tri && limit > 64, [&](auto jtag, const int k4) {
#pragma unroll
                            for (int i = 0; i < R; ++i) {
                                __builtin_amdgcn_sched_barrier(0);
                                El<T>::template mfma_from<decltype(jtag)::value>(acc, a[i], b[i]);
                                __builtin_amdgcn_sched_barrier(0);
                                ldA(a[i], k4 + i + R); ldB(b[i], k4 + i + R);
                            }
                        });
                        GPT_VT(14);
                        __syncthreads();                                  // the image is free again (next sweep's first fill)
                    } else if constexpr (R == 2) {
                        AF a0, a1;
                        v4 b0, b1;
                        ldA(a0, d_lo); ldA(a1, d_lo + 1); ldB(b0, d_lo);
                        tri_loop(std::integral_constant<int, 2>{}, d_lo, limit > d_lo ? limit : d_lo, tri, [&](auto jtag, const int k4) {
                            ldB(b1, k4 + 1);
                            __builtin_amdgcn_sched_barrier(0);
                            El<T>::template mfma_from<decltype(jtag)::value>(acc, a0, b0);
                            __builtin_amdgcn_sched_barrier(0);
                            ldA(a0, k4 + 2); ldB(b0, k4 + 2);
                            __builtin_amdgcn_sched_barrier(0);
                            El<T>::template mfma_from<decltype(jtag)::value>(acc, a1, b1);
                            __builtin_amdgcn_sched_barrier(0);
                            ldA(a1, k4 + 3);
                        });
                    } else {
                        // Both operands R - 1 MFMA blocks ahead.  A wave alone on its SIMD (g = 7 for 112 of its 128 steps) has
                        // 1024 cycles per block, and the B image of a small model's block comes from beyond L2 (32 workgroups x
                        // 0.5 MB per XCD at N = 1024): one block ahead such a wave ran at 1490 cycles per step (r04_small_n.txt).
                        AF a[R];
                        v4 b[R];
#pragma unroll
                        for (int i = 0; i < R; ++i) { ldA(a[i], d_lo + i); ldB(b[i], d_lo + i); }
                        tri_loop(std::integral_constant<int, R>{}, d_lo, limit > d_lo ? limit : d_lo, tri, [&](auto jtag, const int k4) {     // d_lo and limit are multiples of 16, R divides 16
#pragma unroll
                            for (int i = 0; i < R; ++i) {
                                __builtin_amdgcn_sched_barrier(0);
                                El<T>::template mfma_from<decltype(jtag)::value>(acc, a[i], b[i]);
                                __builtin_amdgcn_sched_barrier(0);
                                ldA(a[i], k4 + i + R); ldB(b[i], k4 + i + R);
                            }
                        });
                    }
                }
            }
            GPT_VT(5);
            if (vslot >= 0) {
                // cut sweep: this part's 512 x 64 partial product goes to vslab, [vslot][wave][r*4+t][lane] (k_var_combine)
                v4* dst = reinterpret_cast<v4*>(vslab) + ((size_t)vslot * 8 + w) * (16 * 64) + lane;
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int t = 0; t < 4; ++t) dst[(r * 4 + t) * 64] = acc[r][t];
            } else if (GPT_ABL != 9) {
                // whole sweep: fold this wave's 64 rows of V into the per-column sums
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const T v = acc[r][t][e];
                            ssq[t] += v * v;
                            if (CROSS) crs[t] += v * __shfl(v, lane & ~(CPQ - 1));
                        }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int t = 0; t < 4; ++t) El<T>::keep1(acc[r][t]);
            }
            GPT_VT(6);
        };

        if (flags & VI_GEN) {
            sweep(std::true_type{});
            // every wave's part of the scratch image must have reached L2 before another wave reloads it
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        } else {
            sweep(std::false_type{});
        }
        GPT_VT(7);

        if (slot >= 0) {
            // rows of a column are spread over the 4 lane groups lk = 0..3 and over the 8 waves
            T s2[4], cr[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s2[t] = ssq[t]; cr[t] = crs[t];
                s2[t] += __shfl_xor(s2[t], 16); s2[t] += __shfl_xor(s2[t], 32);
                if (CROSS) { cr[t] += __shfl_xor(cr[t], 16); cr[t] += __shfl_xor(cr[t], 32); }
            }
            if (lk == 0) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    red[0][w][16 * t + lc] = s2[t];
                    red[1][w][16 * t + lc] = CROSS ? cr[t] : (T)0;
                }
            }
            __syncthreads();
            if (threadIdx.x < VAR_SLOT) {
                const int which = threadIdx.x >> 6, cl = threadIdx.x & 63;
                T v = (T)0;
#pragma unroll
                for (int ww = 0; ww < 8; ++ww) v += red[which][ww][cl];
                slab[(size_t)slot * VAR_SLOT + threadIdx.x] = v;
            }
        }
        GPT_VT(8);
    }
#ifdef GPT_VAR_TRACE
    if (vt_wg) vt_wg[1] = vt_realtime();
#endif
}

// The one choice of k_var's instantiation <T, NCOMP, CROSS, KT, DW, KSTAR, HALF>, and its launch with arguments `a`.  A unit
// instantiates one side of it per kernel type: DERIV = false, k* alone (ncomp == 1: every kernel type, gpt_predict.hip), or DERIV =
// true, the derivative-column shapes (the other `ncomp` codes of gpt_common.h: RBF in gpt_predict.hip, Matern 3/2 and 5/2 in
// gpt_predict_matern.hip; Matern 1/2 has none, the API refuses its derivatives).  diag_half: launch_var_t.
template <typename T, int KT, bool DERIV, class... A>
void launch_kvar(int ncomp, bool cross, int D, bool diag_half, dim3 grid, hipStream_t s, A... a) {
    auto one = [&](auto nc, auto cr, auto dw, auto kstar) {
        constexpr int NC = decltype(nc)::value, DW = decltype(dw)::value;
        constexpr bool CR = decltype(cr)::value, KS = decltype(kstar)::value;
        // HALF exists for fp64 alone (launch_var_t), and not: at ncomp == 3 (at the register limit it keeps a spilled pointer inside
        // the lock-step loop), for rows of 16, without the k* column, for Matern derivatives (the plain kernel runs at every model size)
        if constexpr (std::is_same<T, double>::value && NC != 3 && DW != MAX_D && KS && (NC == 1 || KT == KT_RBF)) {
            if (diag_half) { launch_lds<k_var<T, NC, CR, KT, DW, KS, true>>(grid, dim3(512), var_lds_bytes<T>(), s, a...); return; }
        }
        launch_lds<k_var<T, NC, CR, KT, DW, KS, false>>(grid, dim3(512), var_lds_bytes<T>(), s, a...);
    };
    constexpr Bool<true> yes{};
    constexpr Bool<false> no{};
    if constexpr (!DERIV) {
        with_coord_width(D, [&](auto dw) { one(Int<1>{}, no, dw, yes); });
    } else {
        static_assert(KT != KT_MATERN12, "Matern 1/2 has no derivative columns");
        // a fused layout (k*, dk_0 .. dk_{D-1} per query), with the cross products k* . dk_d for d var or without
        auto fused = [&](auto nc, auto dw) { if (cross) one(nc, yes, dw, yes); else one(nc, no, dw, yes); };
        if (ncomp == 3) one(Int<3>{}, no, Int<3>{}, yes);                           // Jacobian variance alone, D <= 3: D columns per query
        else if (ncomp == VAR_NCOMP_DERIV4) one(Int<4>{}, no, Int<WIDE_D>{}, no);   // Jacobian variance alone, D = 4: dk_0 .. dk_3
        else if (ncomp == VAR_NCOMP_DERIV8) one(Int<8>{}, no, Int<WIDE_D>{}, no);   // Jacobian variance alone, D = 8
        else if (ncomp == 4) fused(Int<4>{}, Int<3>{});                             // D <= 3
        else if (ncomp == 8) fused(Int<8>{}, Int<WIDE_D>{});                        // D = 4 .. 7
        else if (D <= WIDE_D) fused(Int<16>{}, Int<WIDE_D>{});                      // D = 8
        else fused(Int<16>{}, Int<MAX_D>{});                                        // D = 9 .. 15
    }
}

// gpt_predict_matern.hip: k_var launches with derivative columns (ncomp > 1) of a Matern 3/2 or 5/2 model
template <typename T>
void launch_var_matern(hipStream_t s, const KernelParams& p, const VarPlanDev& pl, int ncomp, bool cross, dim3 grid,
                       const T* Xs, const T* Wf, const T* Xq, int64_t M, T* slab, T* vslab, T* bscr);

}  // namespace gpt
