// What the two halves of the subset selection share (internal header): the argument struct of the kernels, the sizes the host
// allocates by, and the launcher.  gpt_select.hip holds the kernels; gpt_select_host.hip holds gpt_select_greedy.  Plain C++: the
// sanitizer build compiles it with g++ (host_stub/).
#pragma once
#include "gpt_common.h"

namespace gpt {

constexpr int SEL_NT = 256;              // threads of a sel_column workgroup (4 waves)
constexpr int SEL_MAX_WG = 2048;         // sel_column workgroups = partial maxima the reduction reads

struct SelArgs {
    const double* Xs;        // (N, stride) scaled pool
    double* P;               // (N, mp) pool factor, zero beyond the columns written so far
    double* d;               // (N) residual variance, sklearn's y_var convention (white noise included)
    unsigned char* alive;    // (N) 1 until the row is taken as a pivot
    int* selected;           // (n_total) pivots in insertion order; the first n_pre are prescribed
    double* pivd;            // (n_total) d[pivot] at the moment it was taken
    double* part_d;          // (SEL_MAX_WG) per-workgroup maximum of d over alive rows ...
    int* part_i;             // ... and the lowest index attaining it
    int* fail;               // 0, or 1 + the insertion whose pivot was not positive
    int N, stride, mp, n_pre, ktype;
    double lnc, base_var, alpha;   // log c; c + noise
};

// The whole selection, enqueued without a host round trip: Xs = the pool X (a.N, D) scaled by inv_ls (device, MAX_D) into rows of
// a.stride, d / alive / pivd[0] initialised, then n_total insertions (a column of P each, and the choice of the next pivot).
void launch_sel_schedule(hipStream_t s, const SelArgs& a, const double* X, const double* inv_ls, double* Xs, int D, int n_total);

}  // namespace gpt
