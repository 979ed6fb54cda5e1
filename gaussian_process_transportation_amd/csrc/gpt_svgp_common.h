// What the two SVGP trainers share (internal header; gpt_svgp_train*.hip, gpt_svgp_surface*.hip): the model family's constants
// and the host side of a training call that does not depend on a unit's theta layout.  Each unit keeps its args struct, its
// theta layout (pack / unpack), its workspace and its per-step enqueue.  Plain C++ (the sanitizer build compiles it with g++);
// the device helpers of the whitened ELBO and of Adam are in gpt_svgp_device.h.
#pragma once
#include "gpt_call.h"

namespace gpt {

constexpr int NT = 256;                      // threads per workgroup (16 x 16 in the transport Cholesky's trailing update)
constexpr int64_t SVGP_MAX_STEPS = 1 << 24;  // the failure code packs (step, task) into one int: step * 64 + task
constexpr double JITTER = 1e-4;              // gpytorch's float32 Cholesky jitter (as read); svgp_exact.SVGP_JITTER
constexpr double NOISE_FLOOR = 1e-4;         // GreaterThan(1e-4) on each likelihood noise
constexpr double BETA1 = 0.9, BETA2 = 0.999, ADAM_EPS = 1e-8;
constexpr double LOG_2PI = 1.8378770664093453;

struct SvgpLimits { int max_z, max_t, max_b; };    // inducing points, tasks, rows per batch

// The whole schedule of one call: *_train (apply = 1) and *_elbo_grad (one step, apply = 0).
struct SvgpCall {
    const double *X, *Y;
    int64_t N, num_data;
    int D, T, Zn;
    double *Z, *m, *C, *raw_ls, *raw_os, *raw_noise;       // in / out (out only when apply)
    const int64_t *idx, *bb;
    int64_t n_idx, n_steps;
    double lr;
    int apply;
    double* loss_trace;                                     // n_steps
    double* grads[6];                                       // gZ, gm, gC, g_raw_ls, g_raw_os, g_raw_noise (apply = 0)
};

inline int svgp_check_model(const std::string& w, const SvgpLimits& lim, int D, int T, int Zn) {
    if (D < 1 || D > MAX_DIMS) return fail(GPT_E_ARG, w + ": D must be 1 .. 15, got " + std::to_string(D));
    if (T < 1 || T > lim.max_t) return fail(GPT_E_ARG, w + ": T (tasks) must be 1 .. " + std::to_string(lim.max_t) + ", got " + std::to_string(T));
    if (Zn < 1 || Zn > lim.max_z)
        return fail(GPT_E_ARG, w + ": inducing points must be 1 .. " + std::to_string(lim.max_z) + ", got " + std::to_string(Zn));
    return GPT_OK;
}

// Every argument check of a training call that needs no device; n_raw_ls: D (one length-scale vector) or T * D (one per
// task).  *bmax: the largest batch of the schedule.
inline int svgp_validate(const std::string& w, const SvgpCall& c, const SvgpLimits& lim, size_t n_raw_ls, int* bmax) {
    if (!c.X || !c.Y || !c.Z || !c.m || !c.C || !c.raw_ls || !c.raw_os || !c.raw_noise || !c.idx || !c.bb)
        return fail(GPT_E_ARG, w + ": NULL argument");
    if (int rc = svgp_check_model(w, lim, c.D, c.T, c.Zn)) return rc;
    if (c.N < 1 || c.N > INT_MAX || c.num_data < 1) return fail(GPT_E_ARG, w + ": N must be >= 1");
    if (c.n_steps < 1) return fail(GPT_E_ARG, w + ": empty schedule (no optimiser step)");
    if (c.n_steps > SVGP_MAX_STEPS) return fail(GPT_E_ARG, w + ": more than 2^24 optimiser steps in one call");
    if (c.n_idx < 1 || c.bb[0] < 0 || c.bb[c.n_steps] > c.n_idx) return fail(GPT_E_ARG, w + ": batch boundaries outside the index array");
    *bmax = 0;
    for (int64_t s = 0; s < c.n_steps; ++s) {
        const int64_t b = c.bb[s + 1] - c.bb[s];
        if (b < 1 || b > lim.max_b)
            return fail(GPT_E_ARG, w + ": batch " + std::to_string(s) + " has " + std::to_string(b) + " rows (1 .. " + std::to_string(lim.max_b) + ")");
        if (b > *bmax) *bmax = (int)b;
    }
    for (int64_t i = c.bb[0]; i < c.bb[c.n_steps]; ++i)
        if (c.idx[i] < 0 || c.idx[i] >= c.N) return fail(GPT_E_ARG, w + ": schedule index out of range [0, N) at " + std::to_string(i));
    if (!std::isfinite(c.lr) || c.lr < 0) return fail(GPT_E_ARG, w + ": lr must be finite and >= 0");
    const size_t N = c.N, D = c.D, T = c.T, Zn = c.Zn;
    if (!all_finite(c.X, N * D) || !all_finite(c.Y, N * T) || !all_finite(c.Z, Zn * D) || !all_finite(c.m, T * Zn) ||
        !all_finite(c.C, T * Zn * Zn) || !all_finite(c.raw_ls, n_raw_ls) || !all_finite(c.raw_os, T) || !all_finite(c.raw_noise, T + 1))
        return fail(GPT_E_ARG, w + ": non-finite input");
    return GPT_OK;
}

// Device buffers that do not depend on a unit's layout of theta: the data, the schedule, the loss trace, the failure flag,
// and the flat parameter vector with its gradient and Adam moments.
struct SvgpDevice {
    double *X, *Y, *loss, *theta, *grad, *m1, *m2;
    int *idx, *fail;      // fail: INT_MAX, or step * 64 + task of the first non-positive pivot
};

// Allocates them and enqueues the upload of X, Y, the packed theta, the cleared moments and flag, and the schedule's rows
// idx[bb[0] .. bb[n_steps]) as the kernels read them: idx32 (validated: every index fits an int), which the caller keeps
// alive until the stream has drained.
inline int svgp_upload(CallBuffers& buf, const SvgpCall& c, const std::vector<double>& th, std::vector<int>* idx32, SvgpDevice* d) {
    static const int nofail = INT_MAX;
    const size_t nx = (size_t)c.N * c.D, ny = (size_t)c.N * c.T, nt = th.size(), ni = c.bb[c.n_steps] - c.bb[0];
    const hipStream_t s = buf.stream;
    idx32->resize(ni);
    for (size_t i = 0; i < ni; ++i) (*idx32)[i] = (int)c.idx[c.bb[0] + i];
    CALLCHK(buf.alloc(&d->X, nx));
    CALLCHK(buf.alloc(&d->Y, ny));
    CALLCHK(buf.alloc(&d->idx, ni));
    CALLCHK(buf.alloc(&d->loss, (size_t)c.n_steps));
    CALLCHK(buf.alloc(&d->fail, 1));
    for (double** p : {&d->theta, &d->grad, &d->m1, &d->m2}) CALLCHK(buf.alloc(p, nt));
    CALLCHK(hipMemcpyAsync(d->X, c.X, nx * 8, hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(d->Y, c.Y, ny * 8, hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(d->idx, idx32->data(), ni * sizeof(int), hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(d->fail, &nofail, sizeof(int), hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(d->theta, th.data(), nt * 8, hipMemcpyHostToDevice, s));
    CALLCHK(hipMemsetAsync(d->m1, 0, nt * 8, s));
    CALLCHK(hipMemsetAsync(d->m2, 0, nt * 8, s));
    return GPT_OK;
}

// After the last launch: waits for the schedule, decodes the failure flag, writes the loss trace and reads the flat vector
// (theta when apply, the gradient otherwise) into `out`.  dst: where the unit scatters it, in the order Z, m, C, raw_ls,
// raw_os, raw_noise: the caller's parameters (apply), or its gradient arrays (any of which may be NULL).
inline int svgp_read_back(const std::string& w, hipStream_t s, const SvgpCall& c, const SvgpDevice& d, std::vector<double>* out,
                          double* dst[6]) {
    CALLCHK(hipGetLastError());
    int failed = INT_MAX;
    std::vector<double> loss(c.n_steps);
    CALLCHK(hipMemcpyAsync(&failed, d.fail, sizeof(int), hipMemcpyDeviceToHost, s));
    CALLCHK(hipMemcpyAsync(loss.data(), d.loss, (size_t)c.n_steps * 8, hipMemcpyDeviceToHost, s));
    CALLCHK(hipMemcpyAsync(out->data(), c.apply ? d.theta : d.grad, out->size() * 8, hipMemcpyDeviceToHost, s));
    CALLCHK(hipStreamSynchronize(s));
    if (failed != INT_MAX)
        return fail(GPT_E_NOT_PD, w + ": non-positive pivot in chol(c_t k(Z,Z) + eps I) at optimiser step " + std::to_string(failed / 64) +
                                      " (task " + std::to_string(failed % 64) + "); parameters left as they were passed");
    if (c.loss_trace)
        for (int64_t i = 0; i < c.n_steps; ++i) c.loss_trace[i] = loss[i];
    double* params[6] = {c.Z, c.m, c.C, c.raw_ls, c.raw_os, c.raw_noise};
    for (int q = 0; q < 6; ++q) dst[q] = c.apply ? params[q] : c.grads[q];
    return GPT_OK;
}

// A *_elbo_grad entry point: one step over the whole of (Xb, Yb) with apply = 0, through the unit's run().
// params: Z, m, C, raw_ls, raw_os, raw_noise (read only); grads in the same order.
inline int svgp_elbo_grad(int (*run)(int device, const char* who, const SvgpCall& c), const char* who, const SvgpLimits& lim, int device,
                          const double* Xb, const double* Yb, int64_t b, int64_t num_data, int D, int T, int Zn,
                          const double* const params[6], double* loss, double* const grads[6]) {
    if (b < 1 || b > lim.max_b)
        return fail(GPT_E_ARG, std::string(who) + ": batch size must be 1 .. " + std::to_string(lim.max_b) + ", got " + std::to_string(b));
    std::vector<int64_t> idx(b);
    for (int64_t i = 0; i < b; ++i) idx[i] = i;
    const int64_t bb[2] = {0, b};
    double* p[6];
    for (int q = 0; q < 6; ++q) p[q] = const_cast<double*>(params[q]);
    SvgpCall c{};
    c.X = Xb; c.Y = Yb; c.N = b; c.num_data = num_data; c.D = D; c.T = T; c.Zn = Zn;
    c.Z = p[0]; c.m = p[1]; c.C = p[2]; c.raw_ls = p[3]; c.raw_os = p[4]; c.raw_noise = p[5];
    c.idx = idx.data(); c.bb = bb; c.n_idx = b; c.n_steps = 1; c.lr = 0.0; c.apply = 0; c.loss_trace = loss;
    for (int q = 0; q < 6; ++q) c.grads[q] = grads[q];
    return run(device, who, c);
}

}  // namespace gpt
