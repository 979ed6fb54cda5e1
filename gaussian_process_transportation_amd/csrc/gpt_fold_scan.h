// What the two halves of the fold scan share (internal header): the kernels' argument struct, the layout of a tile's partial
// reductions and the launchers.  gpt_fold_scan.hip holds the kernels and defines the launchers; gpt_fold_scan_host.hip holds
// gpt_batch_fold_scan.  Plain C++: the sanitizer build compiles it with g++ (host_stub/).
#pragma once
#include "gpt_batch.h"

namespace gpt {

constexpr int FS_MAX_D = 3;              // the map is a displacement of a space of at most 3 dimensions (O = D)
constexpr int FS_PART_D = 3;             // doubles of a tile's partial: min det, sum err, max err
constexpr int FS_PART_I = 2;             // ints of a tile's partial: query index of the minimum, count of det <= 0

struct FoldScanArgs {
    // the models: X (rows, D), Y (rows, D); the surrogate's inputs Xs = X + Y and targets Ys = -Y (rows, D each; null without it)
    const double *X, *Y, *Xs, *Ys, *ls, *c, *noise;    // ls (B, n_ls), c (B), noise (B)
    const int64_t* n_begin;                            // (B + 1)
    const int* list;                                   // fs_factor: the models of this launch
    double *alpha, *beta;                              // (rows, D) each: K^-1 Y, K(Xs)^-1 Ys
    int *status, *sur_status;                          // (B) each; sur_status null without the surrogate
    // the queries: model b scans Xq rows [x_begin, x_begin + M_b), x_begin = shared ? 0 : o_begin[b]; its per-query outputs are
    // rows [o_begin[b], o_begin[b + 1]) of det, z, err
    const double* Xq;
    const int64_t* o_begin;                            // (B + 1)
    const int *tile_model, *tile_q0;                   // per fs_scan workgroup: the model, the first of its BAT_QT queries
    const int* tile_first;                             // (B): the first of model b's ceil(M_b / BAT_QT) tiles, which are consecutive
    double* part;                                      // (tiles, FS_PART_D)
    int* ipart;                                        // (tiles, FS_PART_I)
    double *det, *z, *err;                             // per query, any may be null
    double *min_det, *err_sum, *err_max;               // (B) each
    int64_t *argmin, *n_fold;                          // (B) each
    int D, n_ls, shared, surrogate;
    double jitter;
};

// Factors the models a.list[0 .. n_small + n_large), the source matrix and (a.surrogate) the surrogate's in the same workgroup:
// one launch per size class present, the small class (n <= BAT_SMALL_N) first in the list.
void launch_fs_factor(hipStream_t s, int n_small, int n_large, const FoldScanArgs& a);
// Scans the tiles [0, tiles_small) with the small size class and [tiles_small, tiles_small + tiles_large) with the large one,
// then reduces every model's tiles (one workgroup per model, B of them) to its five numbers.
void launch_fs_scan(hipStream_t s, int tiles_small, int tiles_large, int64_t B, const FoldScanArgs& a);

}  // namespace gpt
