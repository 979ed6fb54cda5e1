// gpt_rollout_policy / gpt_rollout_policy_dev (include/gpt_hip.h): argument checks, the launches of one call enqueued back to back,
// the hand-over between the handles' streams, and the chunked staging of the host call (gpt_rollout_call.h, shared with the
// stabilised rollout).  Host code only (the kernel:
// gpt_rollout.hip, reached through the launcher of gpt_rollout.h; the handles: through the accessors of gpt_stage.h), so it also
// compiles under g++ against host_stub/ and runs under the sanitizers (make host-oneshot-asan).  The resources of the call
// (CALL_ROLLOUT) are held by the handle of the LAST stage, or by the dynamics' when there is no stage; its events: ev[j] the j-th
// other stream has caught up, ev[2 CHAIN_MAX] the last launch is done.
#include "gpt_rollout_call.h"

using namespace gpt;

namespace {

// the arguments of both entry points (host or device pointers alike), arrays indexed by RO_*
struct RolloutCall : RolloutCallBase {
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

// what both entry points refuse, in the order of the header's list; fills the views
int rollout_check(const char* who, const gpt_chain_stage* stages, RolloutCall& c) {
    const std::string w(who);
    if (int rc = chain_check_models(w, stages, 0, c)) return rc;
    return rollout_check_args(w, c, c.arr[RO_Y0] && c.arr[RO_PATH] && c.arr[RO_STEPS] && c.arr[RO_STATUS]);
}

// every pointer of `c` in device memory; enqueues the whole call, waits for nothing
int rollout_dev(const RolloutCall& c) {
    RolloutArgs a{};
    a.Y0 = static_cast<const double*>(c.arr[RO_Y0]); a.X0 = static_cast<const double*>(c.arr[RO_X0]);
    a.path = static_cast<double*>(c.arr[RO_PATH]); a.vel = static_cast<double*>(c.arr[RO_VEL]); a.x = static_cast<double*>(c.arr[RO_X]);
    a.steps_done = static_cast<int*>(c.arr[RO_STEPS]); a.status = static_cast<int*>(c.arr[RO_STATUS]);
    return rollout_enqueue(c, a, rollout_steps_per_launch(ROLLOUT_STEPS_PER_LAUNCH), [&](hipStream_t s, int D) { launch_rollout(s, D, a); });
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
    return rollout_host_chunks<RO_COUNT>(w, c, row_bytes, rollout_dev);
}
