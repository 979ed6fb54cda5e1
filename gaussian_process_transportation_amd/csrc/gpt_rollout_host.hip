// gpt_rollout_policy / gpt_rollout_policy_dev (include/gpt_hip.h): argument checks, the launches of one call enqueued back to back,
// the hand-over between the handles' streams, and the chunked staging of the host call.  Host code only (the kernel:
// gpt_rollout.hip, reached through the launcher of gpt_rollout.h; the handles: through the accessors of gpt_stage.h), so it also
// compiles under g++ against host_stub/ and runs under the sanitizers (make host-oneshot-asan).  The resources of the call
// (CALL_ROLLOUT) are held by the handle of the LAST stage, or by the dynamics' when there is no stage; its events: ev[j] the j-th
// other stream has caught up, ev[2 CHAIN_MAX] the last launch is done.
#include "gpt_rollout.h"
#include "gpt_chain_check.h"

#include <cstdlib>

using namespace gpt;

namespace {

// the arguments of both entry points (host or device pointers alike), arrays indexed by RO_*
struct RolloutCall : ChainModels {
    int64_t M = 0, T = 0;
    double dt = 0.0, rtol = 0.0;
    int max_passes = 0;
    void* arr[RO_COUNT] = {};            // (the inputs RO_Y0, RO_X0 are only read)
};

// bytes per trajectory, by RO_*
size_t row_bytes(int which, size_t D, size_t T) {
    switch (which) {
        case RO_STEPS: case RO_STATUS: return sizeof(int);
        case RO_PATH: return (T + 1) * D * sizeof(double);
        case RO_VEL: case RO_X: return T * D * sizeof(double);
        default: return D * sizeof(double);
    }
}

// steps a launch advances a trajectory by: a long rollout is many short kernels, never one long-running one
int steps_per_launch() {
    if (const char* e = std::getenv("GPT_ROLLOUT_STEPS_PER_LAUNCH")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= INT_MAX) return (int)v;
    }
    return ROLLOUT_STEPS_PER_LAUNCH;
}

// what both entry points refuse, in the order of the header's list; fills the views
int rollout_check(const char* who, const gpt_chain_stage* stages, RolloutCall& c) {
    const std::string w(who);
    if (int rc = chain_check_models(w, stages, 0, c)) return rc;
    if (int rc = chain_check_solver(w, c.rtol, c.max_passes)) return rc;
    if (c.T < 0) return fail(GPT_E_ARG, w + ": n_steps must be >= 0");
    if (!std::isfinite(c.dt) || c.dt == 0.0) return fail(GPT_E_ARG, w + ": dt must be finite and not zero");
    if (c.M < 0 || c.M >= ((int64_t)1 << 31)) return fail(GPT_E_ARG, w + ": M must be 0 .. 2^31 - 1");
    if (c.T >= ((int64_t)1 << 31) || c.M * (c.T + 1) >= ((int64_t)1 << 31))
        return fail(GPT_E_ARG, w + ": M (n_steps + 1), the rows of path, must be below 2^31");
    if (c.M > 0 && (!c.arr[RO_Y0] || !c.arr[RO_PATH] || !c.arr[RO_STEPS] || !c.arr[RO_STATUS]))
        return fail(GPT_E_ARG, w + ": y0, path, steps_done and status must not be NULL");
    return GPT_OK;
}

// every pointer of `c` in device memory; enqueues the whole call, waits for nothing
int rollout_dev(const RolloutCall& c) {
    gpt_handle* const owner = c.owner();
    CallResources* const res = call_resources(owner, CALL_ROLLOUT, CALL_EVENTS);
    if (!res) return GPT_E_HIP;
    const Event *ev_in = res->ev, &ev_done = res->ev[2 * CHAIN_MAX];
    hipStream_t s = c.owner_view().stream;
    const size_t D = c.owner_view().p.D;
    const int T = (int)c.T, per = steps_per_launch();
    RolloutArgs a{};
    a.M = c.M; a.K = c.K;
    chain_kernel_models(c, a.st, a.dyn);
    a.Y0 = static_cast<const double*>(c.arr[RO_Y0]); a.X0 = static_cast<const double*>(c.arr[RO_X0]);
    a.rtol = c.rtol; a.max_passes = c.max_passes; a.dt = c.dt; a.T = T;
    a.path = static_cast<double*>(c.arr[RO_PATH]); a.vel = static_cast<double*>(c.arr[RO_VEL]); a.x = static_cast<double*>(c.arr[RO_X]);
    a.steps_done = static_cast<int*>(c.arr[RO_STEPS]); a.status = static_cast<int*>(c.arr[RO_STATUS]);
    if (T > per) {                                    // more than one launch: the last x of every trajectory is carried between them
        CALLCHK(reserve(res->scratch[0], (size_t)c.M * D * sizeof(double), s));
        a.state = res->scratch[0];
    }
    hipStream_t other[CHAIN_MAX];
    if (int rc = chain_wait_for_others(c, s, ev_in, other)) return rc;
    // back to back, no host read in between: a trajectory that has ended costs a later launch one wave that returns at once
    for (int t = 0;;) {
        a.t_begin = t;
        a.t_end = T - t > per ? t + per : T;
        launch_rollout(s, (int)D, a);
        t = a.t_end;
        if (t >= T) break;
    }
    // the other streams go on once their models have been read
    if (c.K > 0) {
        CALLCHK(hipEventRecord(ev_done, s));
        for (int j = 0; j < c.K; ++j) CALLCHK(hipStreamWaitEvent(other[j], ev_done, 0));
    }
    CALLCHK(hipGetLastError());
    return GPT_OK;
}

}  // namespace

#define ROLLOUT_CALL(c)                                                                                                        \
    RolloutCall c;                                                                                                             \
    c.K = K; c.h_dyn = h_dyn; c.M = M; c.T = n_steps; c.dt = dt; c.rtol = rtol; c.max_passes = max_passes;                     \
    {                                                                                                                          \
        void* const all[RO_COUNT] = {const_cast<double*>(y0), const_cast<double*>(x0), path, vel, x, steps_done, status};      \
        for (int k = 0; k < RO_COUNT; ++k) c.arr[k] = all[k];                                                                  \
    }

extern "C" int gpt_rollout_policy_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0, int64_t M,
                                      int64_t n_steps, double dt, double rtol, int max_passes, double* path, double* vel, double* x,
                                      int* steps_done, int* status) {
    ROLLOUT_CALL(c);
    if (int rc = rollout_check("gpt_rollout_policy_dev", stages, c)) return rc;
    if (M == 0) return GPT_OK;
    return rollout_dev(c);
}

extern "C" int gpt_rollout_policy(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0, int64_t M,
                                  int64_t n_steps, double dt, double rtol, int max_passes, double* path, double* vel, double* x,
                                  int* steps_done, int* status) {
    ROLLOUT_CALL(c);
    const std::string w = "gpt_rollout_policy";
    if (int rc = rollout_check(w.c_str(), stages, c)) return rc;
    if (M == 0) return GPT_OK;
    const size_t D = c.owner_view().p.D, T = (size_t)n_steps;
    bool finite = all_finite(y0, (size_t)M * D) && (!x0 || all_finite(x0, (size_t)M * D)) && std::isfinite(rtol);
    for (int k = 0; k < K && finite; ++k) finite = affine_finite(c.g[k], D) && std::isfinite(c.scale[k]);
    if (!finite) return fail(GPT_E_ARG, w + ": y0 / x0 / the affine parts / rtol contain NaN or infinity");
    gpt_handle* const owner = c.owner();
    CallResources* const res = call_resources(owner, CALL_ROLLOUT, CALL_EVENTS);
    if (!res) return GPT_E_HIP;
    // a chunk holds about ROLLOUT_CHUNK_ROWS path rows, whatever T is
    const int64_t chunk = std::max<int64_t>(1, ROLLOUT_CHUNK_ROWS / (n_steps + 1));
    ChunkStreams q;
    if (int rc = handle_copy_stream(owner, !one_chunk(M, chunk), &q)) return rc;
    if (int rc = upload_affine(*res, CHAIN_MAX, c.g, K, D, q.s)) return rc;
    // only what the caller asked for is staged and crosses the bus (with T = 0 vel and x have no rows)
    StagedArray table[RO_COUNT];
    for (int k = 0; k < RO_COUNT; ++k) {
        const size_t rb = row_bytes(k, D, T);
        table[k] = StagedArray{rb ? c.arr[k] : nullptr, rb, k < RO_INPUTS, 1};
    }
    return run_chunked(res->st, q, table, M, [&](void* const* dev, int64_t m) {
        RolloutCall d = c;
        d.M = m;
        for (int k = 0; k < K; ++k) d.g[k] = affine_slot(res->affine, k);
        std::copy(dev, dev + RO_COUNT, d.arr);
        return rollout_dev(d);
    }, chunk);
}
