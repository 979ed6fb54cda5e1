// gpt_rollout_pathwise / gpt_rollout_pathwise_dev (include/gpt_hip.h): argument checks, the launches of one call enqueued back to
// back, the hand-over between the handles' streams, and the chunked staging of the host call: gpt_rollout_call.h, shared with the
// other rollouts; here the array table (three inputs with a row per path: y0, x0, func), the refusals of its own, and what the
// functions bring, which has no row per path and is uploaded once per host call: the weights, packed into one [NP][4] image per
// function (the layout of a model's A4), the frequencies and the amplitudes.  Host code only (the kernel: gpt_rollout_pathwise.hip,
// reached through the launcher of gpt_rollout_pathwise.h; the handles: through the accessors of gpt_stage.h), so it also compiles
// under g++ against host_stub/ and runs under the sanitizers (make host-oneshot-asan).  The call shares the resources of
// gpt_rollout_policy (CALL_ROLLOUT) on the handle of the LAST stage, or on the dynamics' when there is no stage.  Its scratch
// there: [0] the guesses carried between launches (gpt_rollout_call.h), and of the host call [1] the weight images, [2] the
// frequencies, [3] the amplitudes.
#include "gpt_rollout_pathwise.h"
#include "gpt_rollout_call.h"

using namespace gpt;

namespace {

// the arguments of both entry points (host or device pointers alike), arrays indexed by RW_*
struct PathwiseCall : RolloutCallBase {
    int64_t S = 0, J = 0;
    const double* weights = nullptr;     // host entry: (S,N,D); device entry and chunks: [S][NP][4]
    const double* omega = nullptr;       // (J,D)
    const double* amp = nullptr;         // (S,J,2,D)
    void* arr[RW_COUNT] = {};            // (the inputs RW_Y0, RW_X0, RW_FUNC are only read)
};

// bytes per path, by RW_*
size_t row_bytes(int which, size_t D, size_t T) {
    switch (which) {
        case RW_FUNC: case RW_STEPS: case RW_STATUS: return sizeof(int);
        case RW_PATH: return (T + 1) * D * sizeof(double);
        case RW_VEL: case RW_X: case RW_F: return T * D * sizeof(double);
        default: return D * sizeof(double);
    }
}

// paths a chunk of the host call may hold at most, when the environment sets a limit (tests: a chunk boundary at a small M)
int64_t chunk_limit() {
    if (const char* e = std::getenv("GPT_ROLLOUT_PATHWISE_CHUNK")) {
        const long long v = std::strtoll(e, nullptr, 10);
        if (v >= 1) return (int64_t)v;
    }
    return 0;
}

// what both entry points refuse, in the order of the header's list; fills the views
int pathwise_check(const std::string& w, const gpt_chain_stage* stages, PathwiseCall& c) {
    if (int rc = chain_check_models(w, stages, 0, c)) return rc;
    if (c.S < 1 || c.S > INT_MAX) return fail(GPT_E_ARG, w + ": S, the number of functions, must be 1 .. 2^31 - 1");
    if (c.J < 0 || c.J > PATHWISE_MAX_FREQ)
        return fail(GPT_E_ARG, w + ": J must be 0 .. " + std::to_string(PATHWISE_MAX_FREQ) + " (GPT_PATHWISE_MAX_FREQ) frequencies, got " +
                                   std::to_string(c.J));
    if (int rc = rollout_check_args(w, c, c.arr[RW_Y0] && c.arr[RW_PATH] && c.arr[RW_STEPS] && c.arr[RW_STATUS])) return rc;
    if (c.M > 0 && !c.arr[RW_FUNC]) return fail(GPT_E_ARG, w + ": func must not be NULL");
    if (c.M > 0 && !c.weights) return fail(GPT_E_ARG, w + ": weights must not be NULL");
    if (c.M > 0 && c.J > 0 && (!c.omega || !c.amp)) return fail(GPT_E_ARG, w + ": omega and amp must not be NULL when J > 0");
    return GPT_OK;
}

// every pointer of `c` in device memory, the weights as images; enqueues the whole call, waits for nothing
int pathwise_dev(const PathwiseCall& c) {
    RolloutPathwiseArgs pa{};
    RolloutArgs& a = pa.r;
    a.Y0 = static_cast<const double*>(c.arr[RW_Y0]); a.X0 = static_cast<const double*>(c.arr[RW_X0]);
    a.path = static_cast<double*>(c.arr[RW_PATH]); a.vel = static_cast<double*>(c.arr[RW_VEL]); a.x = static_cast<double*>(c.arr[RW_X]);
    a.steps_done = static_cast<int*>(c.arr[RW_STEPS]); a.status = static_cast<int*>(c.arr[RW_STATUS]);
    pa.func = static_cast<const int*>(c.arr[RW_FUNC]);
    pa.S = (int)c.S; pa.J = (int)c.J;
    pa.image = (size_t)c.v_dyn.p.NP * 4;
    pa.V4 = c.weights; pa.omega = c.omega; pa.amp = c.amp;
    pa.f = static_cast<double*>(c.arr[RW_F]);
    return rollout_enqueue(c, a, rollout_steps_per_launch(ROLLOUT_PATHWISE_STEPS_PER_LAUNCH),
                           [&](hipStream_t st, int D) { launch_rollout_pathwise(st, D, pa); });
}

// `n` doubles of the host call into scratch buffer `k` of the call's resources, there when the function returns
int upload(CallResources& res, int k, const double* host, size_t n, hipStream_t s, const double** dev) {
    *dev = nullptr;
    if (n == 0) return GPT_OK;
    CALLCHK(reserve(res.scratch[k], n * sizeof(double), s));
    CALLCHK(hipMemcpyAsync(res.scratch[k], host, n * sizeof(double), hipMemcpyHostToDevice, s));
    CALLCHK(hipStreamSynchronize(s));
    *dev = res.scratch[k];
    return GPT_OK;
}

}  // namespace

#define PATHWISE_CALL(c)                                                                                                        \
    PathwiseCall c;                                                                                                             \
    c.K = K; c.h_dyn = h_dyn; c.M = M; c.T = n_steps; c.dt = dt; c.rtol = rtol; c.max_passes = max_passes;                      \
    c.S = S; c.J = J; c.weights = weights; c.omega = omega; c.amp = amp;                                                        \
    {                                                                                                                           \
        void* const all[RW_COUNT] = {const_cast<double*>(y0), const_cast<double*>(x0), const_cast<int*>(func), path, vel, x, f, steps_done, \
                                     status};                                                                                   \
        for (int k = 0; k < RW_COUNT; ++k) c.arr[k] = all[k];                                                                   \
    }

extern "C" int gpt_rollout_pathwise_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0,
                                        const int* func, int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, int64_t S,
                                        const double* weights, int64_t J, const double* omega, const double* amp, double* path, double* vel,
                                        double* x, double* f, int* steps_done, int* status) {
    PATHWISE_CALL(c);
    if (int rc = pathwise_check("gpt_rollout_pathwise_dev", stages, c)) return rc;
    if (M == 0) return GPT_OK;
    return pathwise_dev(c);
}

extern "C" int gpt_rollout_pathwise(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0,
                                    const int* func, int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, int64_t S,
                                    const double* weights, int64_t J, const double* omega, const double* amp, double* path, double* vel,
                                    double* x, double* f, int* steps_done, int* status) {
    PATHWISE_CALL(c);
    const std::string w = "gpt_rollout_pathwise";
    if (int rc = pathwise_check(w, stages, c)) return rc;
    if (M == 0) return GPT_OK;
    const size_t D = c.owner_view().p.D, N = (size_t)c.v_dyn.p.N, NP = (size_t)c.v_dyn.p.NP, nS = (size_t)S, nJ = (size_t)J;
    for (int64_t m = 0; m < M; ++m)
        if (func[m] < 0 || func[m] >= S)
            return fail(GPT_E_ARG, w + ": func[" + std::to_string(m) + "] = " + std::to_string(func[m]) + " is not one of the " + std::to_string(S) +
                                       " functions");
    if (!all_finite(weights, nS * N * D) || (J > 0 && (!all_finite(omega, nJ * D) || !all_finite(amp, nS * nJ * 2 * D))))
        return fail(GPT_E_ARG, w + ": weights / omega / amp contain NaN or infinity");
    // one image per function in the layout of the model's alpha rows: row n = (V[n, 0 .. D - 1], 0 ..), zero rows from N to NP
    std::vector<double> image(nS * NP * 4, 0.0);
    for (size_t s = 0; s < nS; ++s)
        for (size_t n = 0; n < N; ++n)
            for (size_t d = 0; d < D; ++d) image[(s * NP + n) * 4 + d] = weights[(s * N + n) * D + d];
    CallResources* const res = call_resources(c.owner(), CALL_ROLLOUT, CALL_EVENTS);
    if (!res) return GPT_E_HIP;
    hipStream_t s = c.owner_view().stream;
    if (int rc = upload(*res, 1, image.data(), image.size(), s, &c.weights)) return rc;
    if (int rc = upload(*res, 2, omega, nJ * D, s, &c.omega)) return rc;
    if (int rc = upload(*res, 3, amp, nS * nJ * 2 * D, s, &c.amp)) return rc;
    return rollout_host_chunks<RW_COUNT>(w, c, row_bytes, pathwise_dev, RW_INPUTS, chunk_limit());
}
