// Arithmetic constants and work decomposition of the residue (int8) variance kernel k_var_i8 (host-only C++, no HIP: the
// plan is replayed on the CPU by tests/test_var_int8_cpu.py through a small program of its own).
//
// The product V = W K*^T of an fp64 single-task model is taken exactly on the int8 matrix cores: both operands are rounded to
// p-bit integers (rows of W against their own power-of-two bound, kernel columns against the prior variance's), the integer
// product is formed modulo 14 pairwise coprime moduli that fit int8 — one int8 GEMM per modulus, int32 sums — and rebuilt by
// Garner's mixed-radix conversion.  DESIGN.md section 4 has the derivation; tests/var_int8_restatement.py restates it in numpy.
//
// Work split.  Every (column block, i-block) pair writes its 128 column sums to a slab slot of its own, [cb][ib], and the
// finalizing kernel adds a column's nbi slots in i-block order: integer partial sums are exact and the fp64 sums have one fixed
// grouping, so ANY assignment of the pairs to workgroups gives the same bits.  The images of the kernel columns are written by a
// kernel of their own (k_i8_gen) for a group of blocks at a time, so the i-blocks of a block can go to several workgroups.
//   * Rounds: while at least P column blocks are left, the next P are a group.  It is dealt as items (block, i-blocks {nbi - 1 - q, q}):
//     nbi + 1 tiles each, ceil(nbi / 2) per block, workgroup b taking items b, b + P, ... (var_i8_group_item).  Workgroups b, b + 8, ...
//     share an XCD; when the pairs per block divide P they hold the same two i-blocks and walk the same tiles of the W planes in
//     step, one copy of that stream in the XCD's L2.
//   * Tail: the ncb_t < P blocks that are left are a group of their own and get floor(P / ncb_t) workgroups each (at most nbi); the
//     i-blocks of a block are dealt to its workgroups in contiguous ranges of about equal cost (var_i8_tail_item).
//   * Launches: a group's images, then its sweeps — GPT_VAR_ROUNDS_PER_LAUNCH / GPT_VAR_ROUNDS_EXACT groups at a time, and
//     GPT_VAR_ITEM_STEPS_PER_LAUNCH item steps of them per launch of the sweep kernel.
#pragma once
#include <cstdint>
#include <cmath>
#include <cstdlib>
#include <vector>
#include "gpt_plan.h"

namespace gpt {

constexpr int I8_NMOD = 14;
constexpr int I8_MODULI[I8_NMOD] = {256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199};
constexpr int I8_COLS = 128;          // columns per column block (8 MFMA column tiles)
constexpr int I8_ROWS = 512;          // rows of an i-block (= WT)
constexpr int I8_KSTEP = 64;          // k per v_mfma_i32_16x16x64_i8
constexpr int I8_MAX_NBI = 32;        // i-blocks of the largest model the path takes (NP <= 16384: p = 47)
constexpr int I8_MIN_BITS = 44;       // below this many bits per operand a model stays on the fp64 kernel
// Cost of an i-block beside its tiles, in tiles: its 14 reductions and its reconstruction, and its share of the first fill (chunk,
// A ring, barrier), which a walk group of two i-blocks (var_i8_walk_iblock) pays once.  Three, as measured when every i-block
// filled for itself; the tail shapes (M = 10^4 .. 65 536) did not ask for another value with the groups.
constexpr int I8_SWEEP_FIXED = 3;

// log2 of the product of the moduli (110.16)
inline double var_i8_log2_modulus() {
    double s = 0;
    for (int j = 0; j < I8_NMOD; ++j) s += std::log2((double)I8_MODULI[j]);
    return s;
}
// bits per operand: NP 2^(2p) < M / 2, so that the integer product is recovered without wrap-around
inline int var_i8_bits(int NP) {
    int lg = 0;
    while (((int64_t)1 << lg) < NP) ++lg;
    return (int)std::floor((var_i8_log2_modulus() - 1.0 - lg) / 2.0);
}
// smallest e with x <= 2^e (x > 0); 0 for x == 0
inline int var_i8_exponent(double x) {
    if (!(x > 0)) return 0;
    int ex;
    const double f = std::frexp(x, &ex);
    return f == 0.5 ? ex - 1 : ex;
}
// whether a model with this geometry can take the path at all (fp64, one task, D <= 3 is checked by the caller)
inline bool var_i8_shape_ok(int NP) {
    return NP >= I8_ROWS && NP % I8_ROWS == 0 && NP / I8_ROWS <= I8_MAX_NBI && var_i8_bits(NP) >= I8_MIN_BITS;
}

// Device images, in bytes: the residue planes of W (one byte per element of the block lower triangle and modulus); per column
// block of a group the planes of its kernel columns (var_i8_image_count of them); and per workgroup the parked residues of a
// walk group's two i-blocks (2 x 512 x 128 elements x 14 bytes; slot u of the group at u x var_i8_park_slot_bytes()).
inline size_t var_i8_plane_bytes(int NP) { const size_t nb = NP / I8_ROWS; return (size_t)I8_NMOD * (nb * (nb + 1) / 2) * I8_ROWS * I8_ROWS; }
inline size_t var_i8_bimg_bytes(int NP) { return (size_t)I8_NMOD * NP * I8_COLS; }
constexpr size_t var_i8_park_slot_bytes() { return (size_t)I8_NMOD * I8_ROWS * I8_COLS; }
constexpr size_t var_i8_park_bytes() { return 2 * var_i8_park_slot_bytes(); }

// Passed by value to the kernels.
struct VarI8PlanDev {
    int64_t ncb;          // column blocks
    int64_t nfull;        // blocks handled whole in rounds (a multiple of P)
    int P, nbi;
    int nparts;           // workgroups per tail block (0: no tail)
    int bounds[I8_MAX_NBI + 1];      // part q of a tail block takes the i-blocks [bounds[q], bounds[q + 1])
    // the part of the plan one launch executes (launch_var_i8: rounds are dealt to several launches, the tail goes with the last)
    int64_t rnd_begin = 0, rnd_end = 0;
    int step_begin = 0, step_end = 0;     // item steps of each of those rounds (var_i8_group_item)
    int with_tail = 1;
};

// Rounds one launch of the sweep kernel takes: the rule of k_var (gpt_plan.h var_rounds_per_launch) with a default of one round.
// The images of every block of a launch exist before it starts (k_i8_gen), so the count is also held to what I8_IMAGE_BUDGET bytes
// of images allow, and to one round at least.
constexpr size_t I8_IMAGE_BUDGET = (size_t)4 << 30;
inline int64_t var_i8_rounds_per_launch(const VarI8PlanDev& d) {
    const int64_t rpl = var_rounds_per_launch(d.nfull / d.P, (int64_t)d.nbi * (d.nbi + 1) / 2, 1);
    const int64_t fit = (int64_t)(I8_IMAGE_BUDGET / ((size_t)d.P * var_i8_bimg_bytes(d.nbi * I8_ROWS)));
    return fit < 1 ? 1 : (rpl > fit ? fit : rpl);
}
// images the launches of this plan need at once: the rounds of one launch, or the tail's blocks (a group of their own)
inline int64_t var_i8_image_count(const VarI8PlanDev& d) {
    return d.nfull > 0 ? var_i8_rounds_per_launch(d) * d.P : d.ncb - d.nfull;
}

inline int var_i8_iblock_cost(int ib) { return ib + 1 + I8_SWEEP_FIXED; }

inline VarI8PlanDev build_var_i8_plan(int64_t ncols, int nbi, int P) {
    VarI8PlanDev d{};
    d.ncb = (ncols + I8_COLS - 1) / I8_COLS;
    d.P = P; d.nbi = nbi;
    d.nfull = d.ncb / P * P;
    const int64_t ncb_t = d.ncb - d.nfull;
    d.nparts = 0;
    for (int q = 0; q <= I8_MAX_NBI; ++q) d.bounds[q] = nbi;
    if (ncb_t == 0) return d;
    int nparts = (int)(P / ncb_t);
    if (nparts > nbi) nparts = nbi;
    if (nparts < 1) nparts = 1;
    d.nparts = nparts;
    // contiguous ranges of about equal cost: boundary q sits where the running cost passes q / nparts of the total, and every
    // part keeps at least one i-block
    int64_t total = 0;
    for (int ib = 0; ib < nbi; ++ib) total += var_i8_iblock_cost(ib);
    d.bounds[0] = 0;
    int ib = 0;
    int64_t cum = 0;
    for (int q = 1; q < nparts; ++q) {
        const int64_t target = total * q / nparts;
        const int lo = d.bounds[q - 1] + 1, hi = nbi - (nparts - q);      // leave one i-block for every later part
        while (ib < hi && (ib < lo || cum + var_i8_iblock_cost(ib) / 2 < target)) cum += var_i8_iblock_cost(ib++);
        d.bounds[q] = ib;
    }
    d.bounds[nparts] = nbi;
    return d;
}

// What workgroup `wg` does in the tail: column block *cb, i-blocks [*ib_lo, *ib_hi); false: nothing.  (The kernel has the same
// three lines; this copy is for the host-side replay.)
inline bool var_i8_tail_item(const VarI8PlanDev& d, int wg, int64_t* cb, int* ib_lo, int* ib_hi) {
    if (d.nparts <= 0) return false;
    const int64_t c = wg / d.nparts;
    if (c >= d.ncb - d.nfull) return false;
    const int q = wg % d.nparts;
    *cb = d.nfull + c; *ib_lo = d.bounds[q]; *ib_hi = d.bounds[q + 1];
    return true;
}

// ---- items of a whole group (round) of P blocks -----------------------------------------------------------------------------
// i-blocks q and nbi - 1 - q have nbi + 1 tiles together, whatever q: a block is npairs = ceil(nbi / 2) items of equal work (at odd
// nbi the middle i-block is an item alone).  Item t of a group is block t / npairs with the i-blocks {nbi - 1 - q, q}, q = t % npairs;
// workgroup wg takes the items wg, wg + P, ...: one per item step, npairs steps per group.  Co-resident workgroups hold consecutive
// items, and when npairs divides P a workgroup keeps its q.  An item is at most two contiguous i-block ranges, [lo[r], hi[r]), walked
// in order r = 0, 1 and downward inside a range (two i-blocks at a time: "the walk of an item" below); a tail part is an item with one range.  img: the block's image among those that
// k_i8_gen wrote for the launch (the blocks of the launch's rounds; the tail's blocks in a launch of their own).
struct VarI8Item {
    int64_t cb, img;
    int lo[2], hi[2];
};
inline int var_i8_npairs(int nbi) { return (nbi + 1) / 2; }
inline VarI8Item var_i8_group_item(const VarI8PlanDev& d, int64_t round, int step, int wg) {
    const int npairs = var_i8_npairs(d.nbi);
    const int64_t t = (int64_t)step * d.P + wg;
    const int q = (int)(t % npairs);
    VarI8Item x{};
    x.cb = round * d.P + t / npairs;
    x.img = x.cb - d.rnd_begin * d.P;
    x.hi[0] = d.nbi - q; x.lo[0] = x.hi[0] - 1;
    x.lo[1] = q; x.hi[1] = q < x.lo[0] ? q + 1 : q;
    return x;
}
// the tail part of workgroup wg as an item; false: nothing
inline bool var_i8_tail_as_item(const VarI8PlanDev& d, int wg, VarI8Item* x) {
    int lo, hi;
    if (!var_i8_tail_item(d, wg, &x->cb, &lo, &hi)) return false;
    x->img = x->cb - d.nfull;
    x->lo[0] = lo; x->hi[0] = hi; x->lo[1] = x->hi[1] = 0;
    return true;
}
// ---- the walk of an item ------------------------------------------------------------------------------------------------------
// The i-blocks of an item in the order of its ranges (r = 0, 1; downward inside a range) are taken two at a time: walk position k
// belongs to walk group k / 2 and parks its residues in slot k % 2.  A pair item is one group, {nbi - 1 - q, q} in that order (the
// middle i-block of an odd nbi alone); a tail part is consecutive twos walked downward, a single i-block left over when its count is
// odd.  Inside a group the moduli are the OUTER loop: for each modulus the sweep of slot 0, then that of slot 1, each reduced and
// parked; the reconstructions follow the last modulus.  Every pair item of a block therefore runs nbi + 1 tiles and two reductions
// per modulus, whatever q: the workgroups that share a block's image (one per XCD) stay in the same plane of it without any
// synchronisation, and the plane is fetched once for all of them.  k_var_i8 calls these two functions itself.
constexpr int var_i8_walk_len(int lo0, int hi0, int lo1, int hi1) { return (hi0 - lo0) + (hi1 - lo1); }
constexpr int var_i8_walk_iblock(int lo0, int hi0, int lo1, int hi1, int k) {
    return k < hi0 - lo0 ? hi0 - 1 - k : hi1 - 1 - (k - (hi0 - lo0));
}
struct VarI8WalkEntry {
    int group, slot, ib;
};
inline std::vector<VarI8WalkEntry> var_i8_item_walk(const VarI8Item& x) {
    std::vector<VarI8WalkEntry> w;
    const int n = var_i8_walk_len(x.lo[0], x.hi[0], x.lo[1], x.hi[1]);
    for (int k = 0; k < n; ++k) w.push_back({k / 2, k % 2, var_i8_walk_iblock(x.lo[0], x.hi[0], x.lo[1], x.hi[1], k)});
    return w;
}
// tiles a walk group runs per modulus: the sum of ib + 1 over its i-blocks
inline int var_i8_group_tiles(const std::vector<VarI8WalkEntry>& w, int group) {
    int t = 0;
    for (const VarI8WalkEntry& e : w)
        if (e.group == group) t += e.ib + 1;
    return t;
}

// Item steps of a group that go into one launch: GPT_VAR_ITEM_STEPS_PER_LAUNCH, read per call (0 or more than npairs: all of them).
// One, measured at N = 8192, M = 500 000 (profiles/var_int8_items_profile.txt: ms per step 235.7 / 236.4 / 238.5 / 239.9 for 1 / 2 / 4 /
// all 8 steps per launch): as with the rounds, a kernel boundary brings the workgroups of an XCD back in step on the A stream.
constexpr int I8_DEFAULT_ITEM_STEPS = 1;
inline int var_i8_item_steps_per_launch(const VarI8PlanDev& d) {
    const int npairs = var_i8_npairs(d.nbi);
    const char* e = std::getenv("GPT_VAR_ITEM_STEPS_PER_LAUNCH");
    const int v = e ? std::atoi(e) : I8_DEFAULT_ITEM_STEPS;
    return v <= 0 || v > npairs ? npairs : v;
}

}  // namespace gpt
