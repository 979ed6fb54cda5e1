// gpt_rollout_sampled / gpt_rollout_sampled_dev (include/gpt_hip.h): argument checks, the launches of one call enqueued back to
// back, the hand-over between the handles' streams, and the chunked staging of the host call: gpt_rollout_call.h, shared with the
// mean and the stabilised rollout; here the array table (three inputs: y0, x0, normals), the refusals of its own, the scratch of a
// call and the kernel's further arguments.  Host code only (the kernel: gpt_rollout_sampled.hip, reached through the launcher of
// gpt_rollout_sampled.h; the handles: through the accessors of gpt_stage.h), so it also compiles under g++ against host_stub/ and
// runs under the sanitizers (make host-oneshot-asan).  The call shares the resources of gpt_rollout_policy (CALL_ROLLOUT) on the
// handle of the LAST stage, or on the dynamics' when there is no stage.  Its scratch there: [0] the guesses carried between
// launches (gpt_rollout_call.h), [1] u of every step, [2] the factor, transposed, [3] the cross products of the step in hand,
// [4] x where the caller does not ask for it (the kernel reads the path's earlier points).
#include "gpt_rollout_sampled.h"
#include "gpt_rollout_call.h"

using namespace gpt;

namespace {

// the arguments of both entry points (host or device pointers alike), arrays indexed by RP_*
struct SampledCall : RolloutCallBase {
    double nugget = 0.0;
    void* arr[RP_COUNT] = {};            // (the inputs RP_Y0, RP_X0, RP_NORMALS are only read)
};

// bytes per path, by RP_*
size_t row_bytes(int which, size_t D, size_t T) {
    switch (which) {
        case RP_STEPS: case RP_STATUS: return sizeof(int);
        case RP_PATH: return (T + 1) * D * sizeof(double);
        case RP_NORMALS: case RP_VEL: case RP_X: case RP_F: return T * D * sizeof(double);
        case RP_PVAR: case RP_CVAR: return T * sizeof(double);
        case RP_CHOL: return T * T * sizeof(double);
        default: return D * sizeof(double);
    }
}

// bytes of device scratch a chunk of the host call may take
double scratch_budget() {
    if (const char* e = std::getenv("GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES")) {
        const double v = std::strtod(e, nullptr);
        if (v >= 1.0 && v <= 0x1p60) return v;
    }
    return ROLLOUT_SAMPLED_SCRATCH_BUDGET;
}

// what both entry points refuse, in the order of the header's list; fills the views
int sampled_check(const char* who, const gpt_chain_stage* stages, SampledCall& c) {
    const std::string w(who);
    if (int rc = chain_check_models(w, stages, 0, c)) return rc;
    if (c.v_dyn.p.N > ROLLOUT_STAB_MAX_N)
        return fail(GPT_E_ARG, w + ": the dynamics has " + std::to_string(c.v_dyn.p.N) + " training points; the sampled rollout keeps the "
                                   "kernel columns of a step in LDS and takes at most " + std::to_string(ROLLOUT_STAB_MAX_N) +
                                   " (larger models: gpt_predict_cov over the path so far, per step, on the host)");
    if (c.T > ROLLOUT_SAMPLED_MAX_T)
        return fail(GPT_E_ARG, w + ": n_steps must be at most " + std::to_string(ROLLOUT_SAMPLED_MAX_T) + " (GPT_ROLLOUT_SAMPLED_MAX_T: a row of "
                                   "the path's factor is held in registers), got " + std::to_string(c.T));
    if (!std::isfinite(c.nugget) || c.nugget < 0.0) return fail(GPT_E_ARG, w + ": nugget must be finite and >= 0");
    if (int rc = rollout_check_args(w, c, c.arr[RP_Y0] && c.arr[RP_PATH] && c.arr[RP_STEPS] && c.arr[RP_STATUS])) return rc;
    if (c.M > 0 && c.T > 0 && !c.arr[RP_NORMALS]) return fail(GPT_E_ARG, w + ": normals must not be NULL");
    return GPT_OK;
}

// every pointer of `c` in device memory; enqueues the whole call, waits for nothing
int sampled_dev(const SampledCall& c, const std::string& w) {
    const int D = c.owner_view().p.D, N = c.v_dyn.p.N;
    const bool own_x = !c.arr[RP_X];
    const double need = 8.0 * sampled_scratch_doubles(c.M, c.T, N, D, own_x);
    gpt_handle* const owner = c.owner();
    CallResources* const res = call_resources(owner, CALL_ROLLOUT, CALL_EVENTS);      // (the owner's device becomes this thread's)
    if (!res) return GPT_E_HIP;
    const size_t wgs = (size_t)((c.M + ROLLOUT_SAMPLED_TILE - 1) / ROLLOUT_SAMPLED_TILE), T = (size_t)c.T, P = (size_t)c.M;
    // bytes of scratch[1 .. 4]: u of every step, the factor, the cross products, x
    const size_t bytes[4] = {wgs * T * sampled_u_rows(N) * 16 * sizeof(double), P * T * sampled_ld((int)T) * sizeof(double),
                             wgs * (T + 1) * 16 * sizeof(double), own_x ? P * T * D * sizeof(double) : 0};
    // what the call will ask of the device: a buffer that has to grow is freed and allocated anew (reserve), so its whole new size,
    // less what freeing it gives back; a buffer that is large enough asks for nothing
    double ask = 0.0;
    for (int k = 0; k < 4; ++k)
        if (bytes[k] > res->scratch[1 + k].bytes) ask += (double)bytes[k] - (double)res->scratch[1 + k].bytes;
    if (ask > 0.0) {
        size_t mem_free = 0, mem_total = 0;
        CALLCHK(hipMemGetInfo(&mem_free, &mem_total));
        if (ask > ROLLOUT_SAMPLED_MEMORY_SHARE * (double)mem_free)
            return fail(GPT_E_ARG, w + ": the call needs " + std::to_string((long long)(need / 1048576.0)) + " MiB of device scratch (u of every "
                                       "step and the factors of the paths), " + std::to_string((long long)(ask / 1048576.0)) + " MiB more than this handle "
                                       "holds: more than " + std::to_string((int)(ROLLOUT_SAMPLED_MEMORY_SHARE * 100)) +
                                       " % of the device's free memory (" + std::to_string((long long)(mem_free / 1048576)) +
                                       " MiB free); fewer paths per call, or the host entry, which chunks them");
    }
    hipStream_t s = c.owner_view().stream;
    for (int k = 0; k < 4; ++k) CALLCHK(reserve(res->scratch[1 + k], bytes[k], s));
    RolloutSampledArgs sa{};
    RolloutArgs& a = sa.r;
    a.Y0 = static_cast<const double*>(c.arr[RP_Y0]); a.X0 = static_cast<const double*>(c.arr[RP_X0]);
    a.path = static_cast<double*>(c.arr[RP_PATH]); a.vel = static_cast<double*>(c.arr[RP_VEL]);
    a.x = own_x ? res->scratch[4].p : static_cast<double*>(c.arr[RP_X]);
    a.steps_done = static_cast<int*>(c.arr[RP_STEPS]); a.status = static_cast<int*>(c.arr[RP_STATUS]);
    sa.Wf = c.v_dyn.Wf; sa.NP = c.v_dyn.p.NP; sa.c = c.v_dyn.p.c; sa.nugget = c.nugget;
    sa.normals = static_cast<const double*>(c.arr[RP_NORMALS]);
    sa.f = static_cast<double*>(c.arr[RP_F]); sa.pvar = static_cast<double*>(c.arr[RP_PVAR]); sa.cvar = static_cast<double*>(c.arr[RP_CVAR]);
    sa.chol = static_cast<double*>(c.arr[RP_CHOL]);
    sa.U = res->scratch[1]; sa.Gt = res->scratch[2]; sa.cb = res->scratch[3];
    return rollout_enqueue(c, a, rollout_steps_per_launch(ROLLOUT_SAMPLED_STEPS_PER_LAUNCH), [&](hipStream_t st, int D_) { launch_rollout_sampled(st, D_, sa); });
}

}  // namespace

#define SAMPLED_CALL(c)                                                                                                         \
    SampledCall c;                                                                                                              \
    c.K = K; c.h_dyn = h_dyn; c.M = M; c.T = n_steps; c.dt = dt; c.rtol = rtol; c.max_passes = max_passes; c.nugget = nugget;   \
    {                                                                                                                           \
        void* const all[RP_COUNT] = {const_cast<double*>(y0), const_cast<double*>(x0), const_cast<double*>(normals), path, vel, x, f, pvar, cvar, \
                                     chol, steps_done, status};                                                                 \
        for (int k = 0; k < RP_COUNT; ++k) c.arr[k] = all[k];                                                                   \
    }

extern "C" int gpt_rollout_sampled_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0,
                                       const double* normals, int64_t M, int64_t n_steps, double dt, double rtol, int max_passes,
                                       double nugget, double* path, double* vel, double* x, double* f, double* pvar, double* cvar,
                                       double* chol, int* steps_done, int* status) {
    SAMPLED_CALL(c);
    const std::string w = "gpt_rollout_sampled_dev";
    if (int rc = sampled_check(w.c_str(), stages, c)) return rc;
    if (M == 0) return GPT_OK;
    return sampled_dev(c, w);
}

extern "C" int gpt_rollout_sampled(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0,
                                   const double* normals, int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, double nugget,
                                   double* path, double* vel, double* x, double* f, double* pvar, double* cvar, double* chol,
                                   int* steps_done, int* status) {
    SAMPLED_CALL(c);
    const std::string w = "gpt_rollout_sampled";
    if (int rc = sampled_check(w.c_str(), stages, c)) return rc;
    if (M == 0) return GPT_OK;
    const size_t D = c.owner_view().p.D;
    if (n_steps > 0 && !all_finite(normals, (size_t)M * (size_t)n_steps * D)) return fail(GPT_E_ARG, w + ": normals contain NaN or infinity");
    // paths per chunk: whole workgroups whose scratch stays within the budget, one workgroup at the least
    const double per_tile = 8.0 * sampled_scratch_doubles(ROLLOUT_SAMPLED_TILE, c.T, c.v_dyn.p.N, (int)D, !x);
    const double tiles = std::floor(scratch_budget() / std::max(per_tile, 1.0));
    const int64_t max_chunk = ROLLOUT_SAMPLED_TILE * (int64_t)std::min(std::max(tiles, 1.0), 0x1p40);
    return rollout_host_chunks<RP_COUNT>(w, c, row_bytes, [&](const SampledCall& d) { return sampled_dev(d, w); }, RP_INPUTS, max_chunk);
}
