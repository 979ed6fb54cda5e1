// What the two halves of the device hyper-parameter search share (internal header): the kernel's argument struct, the layout of
// a run's record and the launcher.  gpt_batch_opt.hip holds bat_optimize and defines the launcher; gpt_batch_opt_host.hip holds
// gpt_batch_optimize and gpt_batch_optimize_bounded.  Plain C++: the sanitizer build compiles it with g++ (host_stub/).
#pragma once
#include "gpt_batch.h"

namespace gpt {

constexpr int64_t BAT_OPT_MAX_R = 1 << 20;      // runs of one call
constexpr int BAT_OPT_MAX_P = 2 + MAX_DIMS;     // components of theta = log [c, l.., noise]
constexpr int BAT_OPT_MAX_LS = 30;              // halvings of one line search
constexpr int BAT_OPT_LIVE = -1;                // status of a run that has not ended (internal; GPT_OPT_* are >= 0)
constexpr int BAT_OPT_CNT = 3;                  // a run's counters: iterations, evaluations, halvings of the current line search

// Doubles of one run's record, P = 2 + n_ls: x, g, d, trial point, trial gradient, H y (P each), H (P x P), f, step length.
// The record lives in global memory: the large size class leaves the CU's LDS no room for it (gpt_batch.hip).
constexpr size_t bat_opt_record(int P) { return (size_t)P * P + 6 * (size_t)P + 2; }

struct BatOptArgs {
    const double *X, *Y, *bounds;       // (rows, D), (rows, O), (P, 2): lo, hi in log space, lo == hi: fixed
    int64_t bounds_stride;              // doubles from a run's bounds to the next run's: 0 (all runs share them) or 2 P
    const int64_t* n_begin;             // (B + 1)
    const int *run_model, *list;        // (R): a run's model; the runs of this launch
    double* rec;                        // (R, bat_opt_record(P))
    int* cnt;                           // (R, BAT_OPT_CNT), zero before a run's first launch
    double *theta, *lml;                // (R, P): the clipped start until the run ends, then its result; (R)
    int *iters, *evals, *status;        // (R) each; status BAT_OPT_LIVE until the run ends
    int D, O, n_ls, max_iter, max_evals, max_ls, evals_per_launch;
    double jitter, pgtol, ftol;
};

// Carries the runs a.list[0 .. n_small + n_large) on by at most a.evals_per_launch objective evaluations each: one launch per
// size class present, the runs of small models (n <= BAT_SMALL_N) first in the list.
void launch_bat_optimize(hipStream_t s, int ktype, int n_small, int n_large, const BatOptArgs& a);

}  // namespace gpt
