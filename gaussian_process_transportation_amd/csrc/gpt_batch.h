// What the two halves of the batched small-GP unit share (internal header): the limits, the kernels' argument structs and the
// launchers.  gpt_batch.hip holds the kernels and defines the launchers; gpt_batch_host.hip holds the entry points and everything
// that validates, packs, allocates, copies and reads back, among it the checks of a batch's geometry that the search's entry
// point (gpt_batch_opt_host.hip) makes too.  Plain C++: the sanitizer build compiles it with g++ (host_stub/).
#pragma once
#include "gpt_common.h"

#include <string>
#include <vector>

namespace gpt {

constexpr int BAT_MAX_N = 128;           // points of one model
constexpr int BAT_SMALL_N = 32;          // ... of the small size class
constexpr int BAT_MAX_O = 16;            // outputs (right-hand sides)
constexpr int64_t BAT_MAX_B = 1 << 20;   // models of one call
constexpr int BAT_QT = 64;               // queries of a bat_predict workgroup = its threads

struct BatArgs {
    const double *X, *Y, *ls, *c, *noise;          // (rows, D), (rows, O), (B, n_ls), (B), (B)
    const int64_t *n_begin, *l_begin, *w_begin;    // (B + 1) each: rows, n^2 images, packed triangles before a model
    const int* list;                               // the models of this launch
    double *L, *alpha, *Wp, *lml, *grad;           // outputs; L, Wp, lml may be null; grad: objective only
    int* status;
    int D, O, n_ls;
    double jitter;
};

struct BatPredArgs {
    const double *X, *ls, *c, *noise, *alpha, *Wp, *Xq;
    const int64_t *n_begin, *w_begin, *q_begin;
    const int *tile_model, *tile_q0;               // per workgroup: the model, the first of its queries
    const int* status;
    double *mean, *var, *J, *Jvar, *dvar;          // any may be null
    int D, O, n_ls;
};

// Factors the models a.list[0 .. n_small + n_large): one launch per size class present, the small class (n <= BAT_SMALL_N)
// first in the list.  obj: the objective (LML and its gradient); otherwise alpha and whichever of L, Wp, lml are not null.
void launch_bat_factor(hipStream_t s, int ktype, bool obj, int n_small, int n_large, const BatArgs& a);
// Predicts the tiles [0, tiles_small) with the small size class and [tiles_small, tiles_small + tiles_large) with the large one.
// der: J, Jvar or dvar is asked for (RBF only).
void launch_bat_predict(hipStream_t s, int ktype, bool der, int tiles_small, int tiles_large, const BatPredArgs& a);

// Host only (gpt_batch_host.hip), for the entry points of this unit and of the search (gpt_batch_opt_host.hip).
// What every call on a ragged batch checks of its geometry, refused under the caller's name w: B, D, O, n_ls, kernel_type,
// alpha_jitter, n_begin (starts at 0, 1 <= n_b <= BAT_MAX_N), X and Y finite.  The pointers are not null (the caller's check).
int check_batch_geometry(const std::string& w, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                         int n_ls, double jitter, int ktype);
// The launch list of `count` items, item i working on model model[i] (null: on model i): those of the small size class first,
// each class in rising order.  Returns how many are small.
int small_class_first(const int64_t* n_begin, const int* model, int64_t count, std::vector<int>& list);

}  // namespace gpt
