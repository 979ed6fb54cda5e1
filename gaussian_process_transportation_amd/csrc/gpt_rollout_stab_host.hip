// gpt_rollout_stabilised / gpt_rollout_stabilised_dev (include/gpt_hip.h): argument checks, the launches of one call enqueued back
// to back, the hand-over between the handles' streams, and the chunked staging of the host call: gpt_rollout_call.h, shared with
// the mean rollout; here the array table, the refusals of its own and the kernel's further arguments.  Host code only (the kernel:
// gpt_rollout_stab.hip, reached through the launcher of gpt_rollout_stab.h; the handles: through the accessors of gpt_stage.h), so
// it also compiles under g++ against host_stub/ and runs under the sanitizers (make host-oneshot-asan).  The call shares the
// resources of gpt_rollout_policy (CALL_ROLLOUT) on the handle of the LAST stage, or on the dynamics' when there is no stage: one
// call at a time runs on a handle's stream.  Its events: ev[j] the j-th other stream has caught up, ev[2 CHAIN_MAX] the last
// launch is done.
#include "gpt_rollout_stab.h"
#include "gpt_rollout_call.h"

using namespace gpt;

namespace {

// the arguments of both entry points (host or device pointers alike), arrays indexed by RS_*
struct StabCall : RolloutCallBase {
    double gain = 0.0, std_offset = 0.0;
    void* arr[RS_COUNT] = {};            // (the inputs RS_Y0, RS_X0 are only read)
};

// bytes per trajectory, by RS_*
size_t row_bytes(int which, size_t D, size_t T) {
    switch (which) {
        case RS_STEPS: case RS_STATUS: return sizeof(int);
        case RS_PATH: return (T + 1) * D * sizeof(double);
        case RS_VEL: case RS_X: case RS_F: case RS_DVAR: return T * D * sizeof(double);
        case RS_VAR: return T * sizeof(double);
        default: return D * sizeof(double);
    }
}

constexpr const char* STAB_MATERN12 =
    ": a Matern 1/2 (nu = 0.5) dynamics is not differentiable at the training points: its variance has no gradient to descend; use "
    "RBF, Matern 3/2 or Matern 5/2";
constexpr const char* STAB_MATERN =
    ": the variance gradient of a Matern dynamics uses the analytic derivatives of its posterior; gpt_set_matern_derivatives(h_dyn, 1) "
    "enables them";

// what both entry points refuse, in the order of the header's list; fills the views
int stab_check(const char* who, const gpt_chain_stage* stages, StabCall& c) {
    const std::string w(who);
    if (int rc = chain_check_models(w, stages, 0, c)) return rc;
    if (int rc = check_model_kind(c.v_dyn, w, ModelCheck{"dynamics", "", STAB_MATERN12, STAB_MATERN})) return rc;
    if (c.v_dyn.p.N > ROLLOUT_STAB_MAX_N)
        return fail(GPT_E_ARG, w + ": the dynamics has " + std::to_string(c.v_dyn.p.N) + " training points; the stabilised rollout keeps the "
                                   "kernel columns of a step in LDS and takes at most " + std::to_string(ROLLOUT_STAB_MAX_N) +
                                   " (larger models: one gpt_predict_all per step on the host)");
    if (!std::isfinite(c.gain) || c.gain < 0.0) return fail(GPT_E_ARG, w + ": gain must be finite and >= 0");
    if (!std::isfinite(c.std_offset)) return fail(GPT_E_ARG, w + ": std_offset must be finite");
    return rollout_check_args(w, c, c.arr[RS_Y0] && c.arr[RS_PATH] && c.arr[RS_STEPS] && c.arr[RS_STATUS]);
}

// every pointer of `c` in device memory; enqueues the whole call, waits for nothing
int stab_dev(const StabCall& c) {
    RolloutStabArgs sa{};
    RolloutArgs& a = sa.r;
    a.Y0 = static_cast<const double*>(c.arr[RS_Y0]); a.X0 = static_cast<const double*>(c.arr[RS_X0]);
    a.path = static_cast<double*>(c.arr[RS_PATH]); a.vel = static_cast<double*>(c.arr[RS_VEL]); a.x = static_cast<double*>(c.arr[RS_X]);
    a.steps_done = static_cast<int*>(c.arr[RS_STEPS]); a.status = static_cast<int*>(c.arr[RS_STATUS]);
    sa.Wf = c.v_dyn.Wf; sa.NP = c.v_dyn.p.NP; sa.c = c.v_dyn.p.c; sa.noise = c.v_dyn.p.noise;
    sa.gain = c.gain; sa.std_offset = c.std_offset;
    sa.f = static_cast<double*>(c.arr[RS_F]); sa.var = static_cast<double*>(c.arr[RS_VAR]); sa.dvar = static_cast<double*>(c.arr[RS_DVAR]);
    return rollout_enqueue(c, a, rollout_steps_per_launch(ROLLOUT_STAB_STEPS_PER_LAUNCH), [&](hipStream_t s, int D) { launch_rollout_stab(s, D, sa); });
}

}  // namespace

#define STAB_CALL(c)                                                                                                            \
    StabCall c;                                                                                                                 \
    c.K = K; c.h_dyn = h_dyn; c.M = M; c.T = n_steps; c.dt = dt; c.rtol = rtol; c.max_passes = max_passes;                      \
    c.gain = gain; c.std_offset = std_offset;                                                                                   \
    {                                                                                                                           \
        void* const all[RS_COUNT] = {const_cast<double*>(y0), const_cast<double*>(x0), path, vel, x, f, var, dvar, steps_done, status}; \
        for (int k = 0; k < RS_COUNT; ++k) c.arr[k] = all[k];                                                                   \
    }

extern "C" int gpt_rollout_stabilised_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0,
                                          int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, double gain, double std_offset,
                                          double* path, double* vel, double* x, double* f, double* var, double* dvar, int* steps_done,
                                          int* status) {
    STAB_CALL(c);
    if (int rc = stab_check("gpt_rollout_stabilised_dev", stages, c)) return rc;
    if (M == 0) return GPT_OK;
    return stab_dev(c);
}

extern "C" int gpt_rollout_stabilised(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0, int64_t M,
                                      int64_t n_steps, double dt, double rtol, int max_passes, double gain, double std_offset, double* path,
                                      double* vel, double* x, double* f, double* var, double* dvar, int* steps_done, int* status) {
    STAB_CALL(c);
    const std::string w = "gpt_rollout_stabilised";
    if (int rc = stab_check(w.c_str(), stages, c)) return rc;
    if (M == 0) return GPT_OK;
    return rollout_host_chunks<RS_COUNT>(w, c, row_bytes, stab_dev);
}
