// The residue (int8) variance kernel k_var_i8 and the kernels around it: the image of W in residue planes, the finalizing sum.
// Arithmetic and work split: gpt_plan_i8.h; derivation and measurements: DESIGN.md section 4.  k_var (gpt_kvar.h) is untouched.
// Residues — of the operands when the planes are written, of the int32 accumulators when a sweep ends — are taken with byte dot
// products (v_dot4_u32_u8) and one fp32 quotient, no fp64 and no fix-up: gpt_residue_i8.h.
//
// Shapes:
//   * v_mfma_i32_16x16x64_i8: A fragment = 16 B per lane, lane l holds row l & 15, k = 16 (l >> 4) + byte; B fragment the same
//     with the column in place of the row; C/D: column l & 15, rows 4 (l >> 4) + e.  Both operand images are written by this
//     file in that order (the k order inside a step only has to be the same on both sides).
//   * A planes: [modulus j][tile (ib, kb), kb <= ib][step s 0..8)[row group g 0..8)[row tile r 0..4)[lane] x 16 B — the tiles of
//     an i-block are consecutive, so a sweep reads one contiguous stream per wave: 4 KiB per step.
//   * B planes: k_i8_gen writes the images of a group of column blocks before their sweeps start (fp64 k*, the generating code of
//     k_var, then 14 residues), one workgroup per (block, 512 sources), 4 waves per SIMD: [block][modulus][step][column tile 0..8)
//     [lane] x 16 B, fragment order.  The sweeps stage an image through a double-buffered LDS chunk of one 512-k tile (64 KiB),
//     one barrier per tile; the next chunk is copied piecewise between the MFMA steps.
//   * k_var_i8, the sweeps: a workgroup (512 threads, 8 waves, 2 per SIMD) takes items (gpt_plan_i8.h): a 128-column block and
//     one or two ranges of i-blocks — in a whole group the pair {nbi - 1 - q, q}, nbi + 1 tiles whatever q; in the tail a
//     contiguous range.  Wave w accumulates the 64 x 128 product of its 64-row group, 4 x 8 MFMA tiles = 128 int32 accumulators
//     per lane.  The i-blocks of an item are walked two at a time (gpt_plan_i8.h, "the walk of an item"), and the moduli are the
//     OUTER loop of such a group: for modulus j the sweep of the group's first i-block, then that of its second, each with the one
//     accumulator set, reduced modulo m_j when the sweep ends and parked as one byte per element (4 elements per dword, in the
//     i-block's slot of a per-workgroup global buffer that only the writing lane reads back); after the 14th the lane rebuilds the
//     128 integers of each i-block (Garner, fp32 — every intermediate is an integer below 2^24 — then Horner in fp64), scales,
//     squares and sums into the slab slot [block][i-block].  Every pair item of a block so runs nbi + 1 tiles per modulus: the
//     workgroups that share the block's image stay in one plane of it.
//   * diagonal tile: row group g has nothing beyond step g; a wave runs an even number of steps there, (g + 2) & ~1 (the A ring
//     below is four deep, indexed by step & 3, and turned back by two slots behind a sweep that ran 2 or 6 of them), row groups
//     paired (0,7)(1,6)(2,5)(3,4) on the SIMDs as in k_var: 10 of 16 steps.
#pragma once
#include "gpt_common.h"
#include "gpt_dispatch.h"
#include "gpt_exp.h"
#include "gpt_plan_i8.h"
#include "gpt_residue_i8.h"

namespace gpt {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int I8_TILE_STEPS = I8_ROWS / I8_KSTEP;                        // 8 steps per 512-k tile
constexpr size_t I8_A_STEP = (size_t)8 * 4 * 64;                         // v4i per step of the A planes (8 row groups x 4 row tiles x 64 lanes)
constexpr size_t I8_B_STEP = (size_t)8 * 64;                             // v4i per step of a B plane (8 column tiles x 64 lanes)
constexpr size_t I8_CHUNK = I8_TILE_STEPS * I8_B_STEP;                   // v4i per LDS chunk: 4096 = 64 KiB
constexpr size_t I8_LDS_BYTES = 2 * I8_CHUNK * sizeof(v4i);              // 128 KiB
constexpr size_t I8_PARK_WORDS = var_i8_park_bytes() / 4;                // dwords of a workgroup's parking buffer

// Timing-only ablation builds (make ablate-i8, tools/gpu_ablate_i8.sh; their outputs are wrong on purpose): 1 A fragments always from
// the sweep's first tile, 2 B chunks always from the image's first chunk, 3 both, 4 no generation, 5 no reduce, park or
// reconstruction, 6 = 3 with the LDS reads of the B fragments hoisted out of the steps as well (MFMAs only); 7 and 8 split the two
// VALU phases into arithmetic and memory: 7 the generation without its plane stores, 8 reduce and reconstruction without the park
// stores and loads.
// 4 and 7 act on k_i8_gen (4: not launched; the sweeps then read images nobody wrote), the others on k_var_i8.
#ifndef GPT_ABL_I8
#define GPT_ABL_I8 0
#endif
constexpr bool I8_ABL_A = GPT_ABL_I8 == 1 || GPT_ABL_I8 == 3 || GPT_ABL_I8 == 6;
constexpr bool I8_ABL_B = GPT_ABL_I8 == 2 || GPT_ABL_I8 == 3 || GPT_ABL_I8 == 6;
constexpr bool I8_ABL_NOGEN = GPT_ABL_I8 == 4;
constexpr bool I8_ABL_NORED = GPT_ABL_I8 == 5;
constexpr bool I8_ABL_NOLDS = GPT_ABL_I8 == 6;
constexpr bool I8_ABL_NOPLANEST = GPT_ABL_I8 == 7;
constexpr bool I8_ABL_NOPARK = GPT_ABL_I8 == 8;

// the 14 residue words of 16 integers (a lane's fragment of one step; |x| <= 2^p, p <= 50), plane j to dst[j * stride].  The
// integers are split into bytes once; a residue is two byte dot products and an fp32 quotient (gpt_residue_i8.h), its byte the
// low byte of the result.  The modulus number is wave-uniform: the table arrives by scalar loads.
template <bool STORE = true>
static __device__ __forceinline__ void i8_store_planes(const double (&x)[16], v4i* __restrict__ dst, const size_t stride) {
    uint32_t lo[16], hi[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) i8_operand_split(x[b], lo[b], hi[b]);
    const I8ResTab& T = i8_res_tab();
#pragma unroll 1
    for (int j = 0; j < I8_NMOD; ++j) {
        uint32_t r[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) r[b] = i8_operand_bits(lo[b], hi[b], T, j);
        v4i o;
#pragma unroll
        for (int v = 0; v < 4; ++v) o[v] = (int)i8_pack_bits(r[4 * v], r[4 * v + 1], r[4 * v + 2], r[4 * v + 3]);
        if (STORE) dst[(size_t)j * stride] = o;
        else asm volatile("" ::"v"(o));
    }
}

// ---- the image of W: row exponents, then the planes --------------------------------------------------------------------------
// Wf (fp64, gpt_fit.hip k_pack_w): tile (ib, kb) at ((ib (ib + 1) / 2 + kb) WT^2, [k4][g][q][lane][p] = W[64 g + 16 (2 q + p) + (lane & 15)][4 k4 + (lane >> 4)].
// Pass 1, one workgroup (256 threads) per (tile, row group): thread th always sees the same row — its maximum over the tile's 128
// k4-steps goes to rowmax[row] (bits of a non-negative double order as unsigned integers).
__global__ __launch_bounds__(256) void k_i8_rowmax(const double* __restrict__ Wf, unsigned long long* __restrict__ rowmax) {
    const int tile = blockIdx.x, g = blockIdx.y, th = threadIdx.x;
    int ib = 0;
    while ((ib + 1) * (ib + 2) / 2 <= tile) ++ib;
    const double* src = Wf + (size_t)tile * WT_TILE_DOUBLES + (size_t)g * 256 + th;
    double mx = 0.0;
    for (int k4 = 0; k4 < WT_K4; ++k4) mx = fmax(mx, fabs(src[(size_t)k4 * WT_STEP_DOUBLES]));
    const int q = th >> 7, lane = (th >> 1) & 63, pp = th & 1;
    const int row = ib * WT + 64 * g + 16 * (2 * q + pp) + (lane & 15);
    if (mx > 0.0) atomicMax(rowmax + row, (unsigned long long)__double_as_longlong(mx));
}
// rowscale[i] = 2^(e_i - p), qscale[i] = 2^(p - e_i), e_i the smallest integer with max_k |W_ik| <= 2^e_i
__global__ __launch_bounds__(256) void k_i8_rowscale(const unsigned long long* __restrict__ rowmax, int NP, int p, double* __restrict__ rowscale,
                                                     double* __restrict__ qscale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NP) return;
    const double mx = __longlong_as_double((long long)rowmax[i]);
    int e = 0;
    if (mx > 0.0) {
        int ex;
        const double f = frexp(mx, &ex);
        e = f == 0.5 ? ex - 1 : ex;
    }
    rowscale[i] = ldexp(1.0, e - p);
    qscale[i] = ldexp(1.0, p - e);
}
// Pass 2, one workgroup per (tile, row group): thread handles the fragments (s, r, lane) of all 14 planes, 8 of them.
__global__ __launch_bounds__(256) void k_i8_planes(const double* __restrict__ Wf, const double* __restrict__ qscale, int ntiles, v4i* __restrict__ planes) {
    const int tile = blockIdx.x, g = blockIdx.y;
    int ib = 0;
    while ((ib + 1) * (ib + 2) / 2 <= tile) ++ib;
    const double* src = Wf + (size_t)tile * WT_TILE_DOUBLES;
    for (int u = threadIdx.x; u < I8_TILE_STEPS * 4 * 64; u += 256) {
        const int lane = u & 63, r = (u >> 6) & 3, s = u >> 8;
        const int lr = lane & 15, lk = lane >> 4;
        const double sc = qscale[ib * WT + 64 * g + 16 * r + lr];
        double x[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int col = 64 * s + 16 * lk + b;                       // column of the tile
            const int k4 = col >> 2, lkk = col & 3;
            x[b] = rint(src[((((size_t)k4 * 8 + g) * 2 + (r >> 1)) * 64 + lkk * 16 + lr) * 2 + (r & 1)] * sc);
        }
        v4i* dst = planes + ((((size_t)tile * I8_TILE_STEPS + s) * 8 + g) * 4 + r) * 64 + lane;
        i8_store_planes(x, dst, (size_t)ntiles * I8_TILE_STEPS * I8_A_STEP);
    }
}

// ---- reconstruction ------------------------------------------------------------------------------------------------------------
// r: the 14 balanced residues of an integer C, |C| < M / 2.  Mixed-radix digits in balanced form (i8_garner_digits,
// gpt_residue_i8.h: fp32, every intermediate an integer below 2^24); C = d_0 + m_0 (d_1 + m_1 (d_2 + ...)).  The leading digits of
// a small C are zero, so the Horner sum keeps the relative accuracy of fp64 (13 roundings at most).
static __device__ __forceinline__ double i8_garner(const float (&r)[I8_NMOD]) {
    float d[I8_NMOD];
    i8_garner_digits(r, d);
    double X = (double)d[I8_NMOD - 1];
#pragma unroll
    for (int i = I8_NMOD - 2; i >= 0; --i) X = fma(X, (double)I8_GARNER.m[i], (double)d[i]);
    return X;
}

// x of lane (lane ^ m) of the wave, `lane` given by the caller (the low six bits count): what __shfl_xor(x, m) returns, without the
// lane number that __shfl_xor derives for itself and hipcc keeps in a register from the kernel's entry on
static __device__ __forceinline__ double i8_lane_xor(const double x, const unsigned lane, const unsigned m) {
    const int at = (int)(((lane & 63u) ^ m) << 2);
    const int lo = __builtin_amdgcn_ds_bpermute(at, __double2loint(x)), hi = __builtin_amdgcn_ds_bpermute(at, __double2hiint(x));
    return __hiloint2double(hi, lo);
}

struct VarI8Args {
    const v4i* planes;            // A planes
    const double* rowscale;       // 2^(e_i - p)
    const double* Xs;             // scaled sources, rows of 4
    const double* Xq;             // queries (M, D)
    int64_t M;
    double* slab;                 // [cb][ib][128]
    v4i* bimg;                    // per-workgroup B planes
    unsigned* park;               // per-workgroup parked residues
    double bq;                    // 2^(p - f): kernel values -> integers
    double colscale;              // 2^(f - p)
    int ntiles;                   // nbi (nbi + 1) / 2
};

// ---- the images of the kernel columns -----------------------------------------------------------------------------------------
// Steps [s_lo, s_hi) of column block cb's image: k* in fp64 as k_var's generating sweep computes it, B' = rint(k* 2^(p - f)), 14
// residue planes.  Wave w generates column tile w; a lane its column's 16 consecutive sources per step.  Columns past M repeat
// column M - 1.  Tt: the exp2 table in LDS.
template <int KT>
static __device__ __forceinline__ void i8_gen_columns(const KernelParams& p, const VarI8Args& a, const int64_t cb, const int w, const int lane,
                                                      const int s_lo, const int s_hi, v4i* __restrict__ bim, const int nst, const double* Tt) {
    constexpr double RS2 = 0.70710678118654752440;
    const int lc = lane & 15, lk = lane >> 4, D = p.D;
    const double lnc = p.lnc;
    const int64_t col = cb * I8_COLS + 16 * w + lc;
    const int64_t mm = col < a.M ? col : a.M - 1;
    const double* qp = a.Xq + mm * D;
    double q[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) q[d] = qp[d < D ? d : 0] * ((d < D) ? p.inv_ls[d] * 0.70710678118654752440 : 0.0);
#pragma unroll 1
    for (int s = s_lo; s < (I8_ABL_NOGEN ? s_lo : s_hi); ++s) {
        const double* xp = a.Xs + (size_t)(I8_KSTEP * s + 16 * lk) * 4;
        double x[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const d4 xs = *reinterpret_cast<const d4*>(xp + 4 * b);
            const double d0 = xs[0] * RS2 - q[0], d1 = xs[1] * RS2 - q[1], d2_ = xs[2] * RS2 - q[2];
            double hh = d0 * d0;
            hh = fma(d1, d1, hh);
            hh = fma(d2_, d2_, hh);
            x[b] = rint(kernel_tab<KT>(hh, lnc, Tt) * a.bq);
        }
        i8_store_planes<!I8_ABL_NOPLANEST>(x, bim + ((size_t)s * 8 + w) * 64 + lane, (size_t)nst * I8_B_STEP);
    }
}

// One workgroup per (column block cb0 + blockIdx.x, i-block blockIdx.y = 512 sources = 8 steps): image blockIdx.x of a.bimg.  A
// streaming VALU-and-store loop without accumulators: 4 waves per SIMD (128 VGPRs), so that the stores of one wave hide behind the
// arithmetic of three others.
template <int KT>
__global__ __launch_bounds__(512, 4) void k_i8_gen(KernelParams p, VarI8Args a, int64_t cb0) {
    __shared__ double Tt[256];
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 256) Tt[tid] = g_exp2_table[tid];
    __syncthreads();
    const int nst = p.NP / I8_KSTEP;
    v4i* const bim = a.bimg + (size_t)blockIdx.x * ((size_t)I8_NMOD * nst * I8_B_STEP);
    const int s_lo = I8_TILE_STEPS * (int)blockIdx.y;
    i8_gen_columns<KT>(p, a, cb0 + blockIdx.x, w, tid & 63, s_lo, s_lo + I8_TILE_STEPS, bim, nst, Tt);
}

// ---- the sweeps --------------------------------------------------------------------------------------------------------------
// where a wave's A fragments come from during one sweep: the sweep's own steps [0, l0) at offset b0 of the A planes (in v4i), then the
// next sweep's [0, l1) at b1, then the one after at b2 (the A ring runs four steps ahead, across the end of a sweep); wave-uniform
struct I8Feed {
    size_t b0, b1, b2;
    int l0, l1;
};
// KT takes no part any more (the images arrive generated); the instantiations keep their names for the ISA checks of tools/.
template <int KT>
__global__ __launch_bounds__(512, 2) void k_var_i8(KernelParams p, VarI8PlanDev pl, VarI8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char i8_lds_raw[];
    v4i* const Bs = reinterpret_cast<v4i*>(i8_lds_raw);                 // [buffer 0..2)[step 0..8)[column tile 0..8)[lane]
    __shared__ double red[8][I8_COLS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, lk = lane >> 4;
    const int g = (w < 4) ? w : (11 - w);                               // row group of this wave: 0,1,2,3,7,6,5,4
    const int nbi = pl.nbi;
    const int nst = p.NP / I8_KSTEP;                                    // steps of a whole B plane
    unsigned* const pk = a.park + (size_t)blockIdx.x * I8_PARK_WORDS;     // (wave-uniform; a lane's word sits at utid + 512 x slot)
    const size_t a_plane = (size_t)a.ntiles * I8_TILE_STEPS * I8_A_STEP;        // v4i per A plane
    // operand streams are addressed as a wave-uniform base (scalar registers) plus a 32-bit lane offset: no 64-bit pointer per lane
    const v4i* const a_group = a.planes + (size_t)g * 256;
    const unsigned ulane = lane, utid = tid;
    const int npairs = (nbi + 1) >> 1, nsteps = pl.step_end - pl.step_begin;
    const int64_t n_items = (pl.rnd_end - pl.rnd_begin) * nsteps;

    for (int64_t it = 0;; ++it) {
        // an item: column block cb, i-blocks [lo0, hi0) then [lo1, hi1), each walked downward (var_i8_group_item, var_i8_tail_item)
        int64_t cb; int lo0, hi0, lo1, hi1;
        if (it < n_items) {
            const int64_t t = (int64_t)(pl.step_begin + (int)(it % nsteps)) * pl.P + blockIdx.x;
            const int q = (int)(t % npairs);
            cb = (pl.rnd_begin + it / nsteps) * pl.P + t / npairs;
            hi0 = nbi - q; lo0 = hi0 - 1; lo1 = q; hi1 = q < lo0 ? q + 1 : q;      // (odd nbi: the middle i-block is alone)
        } else {
            if (it > n_items || !pl.with_tail || pl.nparts <= 0) break;
            const int64_t c = blockIdx.x / pl.nparts;
            if (c >= pl.ncb - pl.nfull) break;
            const int q = blockIdx.x % pl.nparts;
            cb = pl.nfull + c; lo0 = pl.bounds[q]; hi0 = pl.bounds[q + 1]; lo1 = hi1 = 0;
        }
        // the block's image: k_i8_gen wrote it in an earlier kernel of this stream, for the blocks rnd_begin P .. of this launch
        const v4i* const bim = a.bimg + (size_t)(cb - pl.rnd_begin * pl.P) * ((size_t)I8_NMOD * nst * I8_B_STEP);

        // The walk (gpt_plan_i8.h): the item's i-blocks two at a time.  A group of ng = 1 or 2 i-blocks is nsw = 14 ng sweeps, the
        // moduli outermost: sweep sw is modulus sw >> (ng - 1) of the group's i-block sw & (ng - 1), parked in that slot.
        const int nwalk = var_i8_walk_len(lo0, hi0, lo1, hi1);
#pragma unroll 1
        for (int k0 = 0; k0 < nwalk; k0 += 2) {
            const int um = k0 + 1 < nwalk ? 1 : 0;                      // ng - 1: mask of the slot in sw, shift of the modulus
            const int nsw = I8_NMOD << um;
            const int ib0 = var_i8_walk_iblock(lo0, hi0, lo1, hi1, k0);
            const int ib1 = um ? var_i8_walk_iblock(lo0, hi0, lo1, hi1, k0 + 1) : ib0;
            const int nmine = (g + 2) & ~1;                             // steps of the diagonal tile this wave runs (even)
            const int lim0 = I8_TILE_STEPS * ib0 + nmine, lim1 = I8_TILE_STEPS * ib1 + nmine;      // steps of a sweep this wave runs
            const size_t tile0 = (size_t)ib0 * (ib0 + 1) / 2, tile1 = (size_t)ib1 * (ib1 + 1) / 2;
            // The A stream of sweep sw and of the two behind it, worked out once per sweep: a step between the MFMAs then costs two
            // compares and four selects of scalar registers, not the products (plane, tile) of its address.  Past the group's last
            // sweep: that sweep again (a redundant load of its first steps, in bounds).
            auto feed_of = [&](const int sw) -> I8Feed {
                auto base = [&](int x) -> size_t {
                    if (x >= nsw) x = nsw - 1;
                    return (size_t)(x >> um) * a_plane + ((x & um) ? tile1 : tile0) * (I8_TILE_STEPS * I8_A_STEP);
                };
                return I8Feed{base(sw), base(sw + 1), base(sw + 2), (sw & um) ? lim1 : lim0, ((sw + 1) & um) ? lim1 : lim0};
            };
            // A fragments of step S < lim + 4 of a sweep; past the wave's last step: the first steps of the sweeps that follow (lim = 2:
            // steps lim + 2, lim + 3 belong to the sweep after the next)
            auto a_ptr = [&](const I8Feed f, const int S) -> const v4i* {
                const int S1 = S - f.l0, S2 = S1 - f.l1;
                size_t b = f.b0;
                int o = S;
                if (S1 >= 0) { b = f.b1; o = S1; }
                if (S2 >= 0) { b = f.b2; o = S2; }
                if (I8_ABL_A) o &= I8_TILE_STEPS - 1;
                return a_group + (b + (size_t)(unsigned)o * I8_A_STEP);
            };
            // first chunk, once per group: modulus 0, tile 0 -> buffer 0 (the last barrier has passed: both buffers are free)
            {
                v4i t8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) t8[i] = bim[utid + 512 * i];
#pragma unroll
                for (int i = 0; i < 8; ++i) Bs[tid + 512 * i] = t8[i];
            }
            // The A ring: four slots of four row tiles, filled once per group.  A sweep starts with its steps 0 .. 3 in slots 0 .. 3, step s of a tile reads
            // slot s & 3 (a tile has 8 steps), and behind the diagonal tile's `nmine` steps the ring is turned back (below).
            v4i ar[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const v4i* ap = a_ptr(feed_of(0), i);
#pragma unroll
                for (int r = 0; r < 4; ++r) ar[i][r] = ap[ulane + 64 * r];
            }
            __syncthreads();
            v4i acc[4][8];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[r][t] = v4i{0, 0, 0, 0};
            int buf = 0;
            // One tile of a sweep: 8 steps of 32 MFMAs, written as a pipeline in source order and fenced with sched_barrier(0), so
            // that hipcc's counted waits are the ones meant (its scheduler had put six of the eight LDS reads of a step directly
            // in front of the MFMAs that take them, behind an lgkmcnt(0) each; the group-barrier hints did not hold it).
            // FULL: every step runs and a chunk follows — straight-line code, no branch in it: hipcc places its waits by counting
            // the loads in flight, and behind a join of two paths it takes the worse of the two.  Not FULL (the diagonal tile): `nrun`
            // steps, a chunk follows if `more_rt`.  (One straight-line copy per step count of the diagonal tile was built too: the
            // four copies held 65 - 300 spill accesses each, accumulators moved around their join.)
            // Order inside a step:
            //   * piece s + 1 of the next chunk (pieces 0 and 1 in step 0) is requested first, and piece s - 1 is written to LDS behind
            //     the step's MFMAs: a piece has three steps to arrive, the first and the last two, and the tile's closing barrier
            //     waits for a load that is two steps old, not one;
            //   * B fragments go through a register ring of 3: column tile u + 2 is requested from LDS, then the four MFMAs of
            //     tile u are issued — the wait in front of them leaves two reads outstanding.  In a FULL tile the ring runs on
            //     across the steps; only the chunk's last two column tiles have nothing left to request (the next chunk is behind
            //     the barrier);
            //   * the A fragments of step s + 4 are requested behind the MFMAs of step s, straight into the ring slot those have
            //     just read: three whole steps, 96 MFMAs of this wave, lie between the request and the first MFMA that waits for
            //     it (loads return in order: the chunk piece requested in front of step s + 1, which comes from HBM, has had as long).
            auto tile = [&](auto full_tag, const int nrun, const bool more_rt, const I8Feed fd, const int S0, const v4i* nsrc) __attribute__((always_inline)) {
                constexpr bool FULL = decltype(full_tag)::value;
                const bool more = FULL || more_rt;
                if (I8_ABL_B) nsrc = bim;
                const v4i* bcur = Bs + (size_t)buf * I8_CHUNK + lane;
                v4i* bnext = Bs + (size_t)(buf ^ 1) * I8_CHUNK + tid;
                v4i st[3];                                       // pieces of the next chunk on their way to LDS
                v4i bq[3];                                       // B fragments on their way to the MFMAs
                if (I8_ABL_NOLDS) bq[0] = bq[1] = bq[2] = bcur[0];
#pragma unroll
                for (int s = 0; s < I8_TILE_STEPS; ++s) {
                    const bool run = FULL || s < nrun;
                    if (more && s == 0) st[0] = nsrc[utid];
                    if (more && s + 1 < I8_TILE_STEPS) st[(s + 1) % 3] = (nsrc + 512 * (s + 1))[utid];      // (the piece's base in scalar registers)
                    __builtin_amdgcn_sched_barrier(0);
                    if (run) {
                        if (!I8_ABL_NOLDS && (s == 0 || !FULL)) {
                            bq[(8 * s) % 3] = bcur[(8 * s) * 64];
                            bq[(8 * s + 1) % 3] = bcur[(8 * s + 1) * 64];
                        }
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            const int u = 8 * s + t;
                            if (!I8_ABL_NOLDS && (t + 2 < 8 || (FULL && s + 1 < I8_TILE_STEPS))) bq[(u + 2) % 3] = bcur[(u + 2) * 64];
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                acc[r][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ar[s & 3][r], bq[u % 3], acc[r][t], 0, 0, 0);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (more && s > 0) bnext[512 * (s - 1)] = st[(s - 1) % 3];
                    if (run) {
                        const v4i* ap = a_ptr(fd, S0 + s + 4);
#pragma unroll
                        for (int r = 0; r < 4; ++r) ar[s & 3][r] = ap[ulane + 64 * r];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (more) bnext[512 * (I8_TILE_STEPS - 1)] = st[(I8_TILE_STEPS - 1) % 3];
                __syncthreads();
                buf ^= 1;
            };
#pragma unroll 1
            for (int sw = 0; sw < nsw; ++sw) {
                const int j = sw >> um, ib = (sw & um) ? ib1 : ib0;
                unsigned* const pku = pk + ((sw & um) ? I8_PARK_WORDS / 2 : 0);
                const I8Feed fd = feed_of(sw);
#pragma unroll 1
                for (int kb = 0; kb < ib; ++kb)         // full tiles; the next chunk is the next tile of this sweep
                    tile(Bool<true>{}, I8_TILE_STEPS, true, fd, kb * I8_TILE_STEPS, bim + ((size_t)j * nst + (kb + 1) * I8_TILE_STEPS) * I8_B_STEP);
                // diagonal tile; the next chunk is tile 0 of the next sweep's plane: this one again when the group's second i-block
                // comes next, the next modulus otherwise; none behind the group's last sweep
                tile(Bool<false>{}, nmine, sw + 1 < nsw, fd, ib * I8_TILE_STEPS, bim + (size_t)((sw + 1) >> um) * nst * I8_B_STEP);
                // the sweep of modulus j over i-block ib is complete: reduce, park in the i-block's slot (4 elements of a tile per
                // dword), start over
                if (I8_ABL_NORED) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int t = 0; t < 8; ++t) asm volatile("" : "+v"(acc[r][t]));
                } else {
                    const I8ResTab& T = i8_res_tab();
                    // (the lane's park address is rebuilt behind every sweep: hoisted out of the sweeps as a 64-bit pointer per lane it
                    // held two VGPRs across the tiles, which have none to spare — tools/check_isa_spills.py)
                    unsigned ut = utid;
                    asm volatile("" : "+v"(ut));
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            uint32_t rr[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) rr[e] = i8_acc_bits(acc[r][t][e], T, j);
                            const unsigned pw = i8_pack_bits(rr[0], rr[1], rr[2], rr[3]);
                            if (I8_ABL_NOPARK) asm volatile("" ::"v"(pw));
                            else pku[ut + 512u * (unsigned)(j * 32 + r * 8 + t)] = pw;
                            acc[r][t] = v4i{0, 0, 0, 0};
                        }
                }
                // the next sweep's steps 0 .. 3 sit in slots nmine & 3 ..: nmine = 2 or 6 leaves them two slots on.  Turn the ring back
                // (selects, no branch).  Here, behind the reduction, their loads have long returned, and the stores above are
                // younger: they are not waited for.
                const bool turn = (nmine & 2) != 0;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const v4i lo2 = ar[i][r], hi2 = ar[i + 2][r];
                        ar[i][r] = turn ? hi2 : lo2;
                        ar[i + 2][r] = turn ? lo2 : hi2;
                    }
            }
            // ---- all 14 residues of the group's 64 x 128 elements per i-block are parked: rebuild, scale, square, sum per column
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll 1
            for (int u = 0; u <= um; ++u) {
                const int ib = u ? ib1 : ib0;
                const unsigned* const pku = pk + (u ? I8_PARK_WORDS / 2 : 0);
                unsigned ut = utid, ulk = (unsigned)lk;                 // (rebuilt here as above: not kept across the sweeps)
                asm volatile("" : "+v"(ut), "+v"(ulk));
#pragma unroll 1
                for (int t = 0; t < 8; ++t) {
                    double ssq = 0.0;
#pragma unroll 1
                    for (int r = 0; r < (I8_ABL_NORED ? 0 : 4); ++r) {
                        unsigned wd[I8_NMOD];
#pragma unroll
                        for (int j = 0; j < I8_NMOD; ++j) {
                            if (I8_ABL_NOPARK) asm volatile("" : "=v"(wd[j]));
                            else wd[j] = pku[ut + 512u * (unsigned)(j * 32 + r * 8 + t)];
                        }
                        const d4 rs = *reinterpret_cast<const d4*>(a.rowscale + (size_t)ib * I8_ROWS + 64 * g + 16 * r + 4 * ulk);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float res[I8_NMOD];
#pragma unroll
                            for (int j = 0; j < I8_NMOD; ++j) res[j] = (float)((int)(wd[j] << (24 - 8 * e)) >> 24);
                            const double v = i8_garner(res) * rs[e] * a.colscale;
                            ssq = fma(v, v, ssq);
                        }
                    }
                    ssq += i8_lane_xor(ssq, ut, 16);
                    ssq += i8_lane_xor(ssq, ut, 32);
                    if (lk == 0) red[w][16 * t + lc] = ssq;
                }
                __syncthreads();
                if (tid < I8_COLS) {
                    double v = 0.0;
#pragma unroll
                    for (int ww = 0; ww < 8; ++ww) v += red[ww][tid];
                    a.slab[((size_t)cb * nbi + ib) * I8_COLS + tid] = v;
                }
                __syncthreads();                                            // (red is written again: the group's second i-block, the next group)
            }
        }
    }
}

// var[m] = c + noise - sum over the i-blocks, in order, of the column's slots (k_var_finalize's formula)
__global__ __launch_bounds__(I8_COLS) void k_var_i8_finalize(KernelParams p, int nbi, const double* __restrict__ slab, int64_t M,
                                                             const double* __restrict__ hdr, double* __restrict__ var) {
    const int64_t cb = blockIdx.x, m = cb * I8_COLS + threadIdx.x;
    if (m >= M) return;
    double s2 = 0.0;
    for (int ib = 0; ib < nbi; ++ib) s2 += slab[((size_t)cb * nbi + ib) * I8_COLS + threadIdx.x];
    const double v = hdr[16] + p.noise - s2;
    var[m] = v < 0.0 ? 0.0 : v;
}

}  // namespace gpt
