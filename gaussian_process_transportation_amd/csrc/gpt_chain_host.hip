// gpt_pullback_chain / gpt_pullback_chain_dev (include/gpt_hip.h): argument checks, the scratch between the launches, the
// hand-over between the handles' streams, and the chunked staging of the host call.  Host code only (the kernels: gpt_chain.hip,
// reached through the launchers of gpt_chain.h; the handles: through the accessors of gpt_stage.h), so it also compiles under
// g++ against host_stub/ and runs under the sanitizers (make host-oneshot-asan).  The resources of the call (CALL_CHAIN) are held
// by the handle of the LAST stage; its events: ev[j] the j-th other stream has caught up, ev[CHAIN_MAX + j] the variance launch on
// it is done, ev[2 CHAIN_MAX] the velocity launch is done.
#include "gpt_chain_check.h"

using namespace gpt;

namespace {

// the arguments of both entry points (host or device pointers alike), arrays indexed by CH_*
struct ChainCall : ChainModels {
    int64_t M = 0;
    double rtol = 0.0, std_offset = 0.0;
    int max_passes = 0;
    void* arr[CH_COUNT] = {};            // (the inputs CH_Y, CH_X0 are only read)
};

// bytes per query (and per stage, from CH_FIRST_STAGE on), by CH_*
size_t row_bytes(int which, size_t D) {
    switch (which) {
        case CH_STATUS: case CH_STAGE_STATUS: case CH_STAGE_PASSES: return sizeof(int);
        case CH_VAR_DYN: case CH_STAGE_MAP_VAR: case CH_STAGE_RES: case CH_STAGE_DET: return sizeof(double);
        case CH_STAGE_A: return D * D * sizeof(double);
        default: return D * sizeof(double);
    }
}

// what both entry points refuse, in the order of the header's list; fills the views
int chain_check(const char* who, const gpt_chain_stage* stages, ChainCall& c) {
    const std::string w(who);
    if (int rc = chain_check_models(w, stages, 1, c)) return rc;
    if (int rc = chain_check_solver(w, c.rtol, c.max_passes)) return rc;
    if (c.M < 0 || c.M >= ((int64_t)1 << 31)) return fail(GPT_E_ARG, w + ": M must be 0 .. 2^31 - 1");
    if (c.M > 0 && (!c.arr[CH_Y] || !c.arr[CH_VEL] || !c.arr[CH_STATUS])) return fail(GPT_E_ARG, w + ": y, vel and status must not be NULL");
    return GPT_OK;
}

// every pointer of `c` in device memory; enqueues the whole call, waits for nothing
int chain_dev(const ChainCall& c) {
    const int K = c.K;
    gpt_handle* const owner = c.h[K - 1];
    CallResources* const res = call_resources(owner, CALL_CHAIN, CALL_EVENTS);
    if (!res) return GPT_E_HIP;
    const Event *ev_in = res->ev, *ev_var = res->ev + CHAIN_MAX, &ev_mid = res->ev[2 * CHAIN_MAX];
    hipStream_t s = c.v[K - 1].stream;
    const int64_t M = c.M;
    const size_t D = c.v[K - 1].p.D;
    void* const* u = c.arr;
    // which intermediate quantities the outputs asked for consume
    const bool need_var_dyn = u[CH_VAR_DYN] || u[CH_VVAR_DYN];
    const bool need_jvar = u[CH_STAGE_JVAR] || u[CH_VVAR_MAP];
    const bool need_map = u[CH_STAGE_MAP_VAR] || need_jvar;         // map_var and Jvar together: one pass of the 4-column launch
    const bool epilogue = u[CH_VVAR_MAP] || u[CH_VVAR_DYN];
    const bool need_A = u[CH_VVAR_DYN] || (u[CH_VVAR_MAP] && K > 1);
    const MidArray mid[6] = {{CH_X, need_var_dyn, D}, {CH_F, epilogue, D}, {CH_VAR_DYN, need_var_dyn, 1},
                             {CH_STAGE_Z, need_map, K * D}, {CH_STAGE_A, need_A, K * D * D}, {CH_STAGE_JVAR, need_jvar, K * D}};
    double* at[6];
    if (int rc = resolve_scratch(*res, u, mid, M, s, at)) return rc;
    ChainArgs a{};
    a.M = M; a.K = K;
    chain_kernel_models(c, a.st, a.dyn);
    a.Y = static_cast<const double*>(u[CH_Y]); a.X0 = static_cast<const double*>(u[CH_X0]);
    a.rtol = c.rtol; a.max_passes = c.max_passes; a.std_offset = c.std_offset;
    a.x = at[0]; a.f = at[1]; a.vel = static_cast<double*>(u[CH_VEL]); a.status = static_cast<int*>(u[CH_STATUS]);
    a.stage_x = static_cast<double*>(u[CH_STAGE_X]); a.stage_z = at[3]; a.stage_A = at[4];
    a.stage_status = static_cast<int*>(u[CH_STAGE_STATUS]); a.stage_passes = static_cast<int*>(u[CH_STAGE_PASSES]);
    a.stage_residual = static_cast<double*>(u[CH_STAGE_RES]); a.stage_det = static_cast<double*>(u[CH_STAGE_DET]);
    a.var_dyn = at[2]; a.stage_Jvar = at[5];
    a.vel_var_map = static_cast<double*>(u[CH_VVAR_MAP]); a.vel_var_dyn = static_cast<double*>(u[CH_VVAR_DYN]);
    // the other handles, stages 0 .. K-2 and the dynamics: what their streams have enqueued so far (a fit, a gpt_factor_commit)
    // comes first
    hipStream_t other[CHAIN_MAX];
    if (int rc = chain_wait_for_others(c, s, ev_in, other)) return rc;
    launch_chain_velocity(s, (int)D, a);
    // their streams go on once x and the z_k are there and their models have been read
    CALLCHK(hipEventRecord(ev_mid, s));
    for (int j = 0; j < K; ++j) CALLCHK(hipStreamWaitEvent(other[j], ev_mid, 0));
    // each variance launch on its own handle's stream (the variance workspace belongs to the handle), one after the other: every
    // one of them is sized to fill the device, and two of them side by side take longer than one after the other
    hipEvent_t prev = nullptr;
    if (need_var_dyn) {
        if (int rc = gpt_predict_all_dev(c.h_dyn, a.x, M, nullptr, at[2], nullptr, nullptr, nullptr)) return rc;
        CALLCHK(hipEventRecord(ev_var[K - 1], other[K - 1]));
        prev = ev_var[K - 1];
    }
    if (need_map)
        for (int k = 0; k < K; ++k) {
            hipStream_t sk = k + 1 < K ? other[k] : s;
            if (prev) CALLCHK(hipStreamWaitEvent(sk, prev, 0));
            double* const mv = static_cast<double*>(u[CH_STAGE_MAP_VAR]);
            if (int rc = gpt_predict_all_dev(c.h[k], a.stage_z + (size_t)k * M * D, M, nullptr, mv ? mv + (size_t)k * M : nullptr, nullptr,
                                             need_jvar ? at[5] + (size_t)k * M * D : nullptr, nullptr))
                return rc;
            if (k + 1 < K) {
                CALLCHK(hipEventRecord(ev_var[k], sk));
                prev = ev_var[k];
            }
        }
    else if (prev) CALLCHK(hipStreamWaitEvent(s, prev, 0));
    launch_chain_variance(s, (int)D, a);
    CALLCHK(hipGetLastError());
    return GPT_OK;
}

}  // namespace

#define CHAIN_CALL(c)                                                                                                               \
    ChainCall c;                                                                                                                    \
    c.K = K; c.h_dyn = h_dyn; c.M = M; c.rtol = rtol; c.max_passes = max_passes; c.std_offset = std_offset;                         \
    {                                                                                                                               \
        void* const all[CH_COUNT] = {const_cast<double*>(y), const_cast<double*>(x0), x, vel, f, status, var_dyn, vel_var_map,      \
                                     vel_var_dyn, stage_x, stage_z, stage_A, stage_Jvar, stage_map_var, stage_status, stage_passes, \
                                     stage_residual, stage_det};                                                                    \
        for (int k = 0; k < CH_COUNT; ++k) c.arr[k] = all[k];                                                                       \
    }

extern "C" int gpt_pullback_chain_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y, const double* x0, int64_t M,
                                      double rtol, int max_passes, double std_offset, double* x, double* vel, double* f, int* status,
                                      double* var_dyn, double* vel_var_map, double* vel_var_dyn, double* stage_x, double* stage_z,
                                      double* stage_A, double* stage_Jvar, double* stage_map_var, int* stage_status, int* stage_passes,
                                      double* stage_residual, double* stage_det) {
    CHAIN_CALL(c);
    if (int rc = chain_check("gpt_pullback_chain_dev", stages, c)) return rc;
    if (M == 0) return GPT_OK;
    return chain_dev(c);
}

extern "C" int gpt_pullback_chain(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y, const double* x0, int64_t M,
                                  double rtol, int max_passes, double std_offset, double* x, double* vel, double* f, int* status,
                                  double* var_dyn, double* vel_var_map, double* vel_var_dyn, double* stage_x, double* stage_z,
                                  double* stage_A, double* stage_Jvar, double* stage_map_var, int* stage_status, int* stage_passes,
                                  double* stage_residual, double* stage_det) {
    CHAIN_CALL(c);
    const std::string w = "gpt_pullback_chain";
    if (int rc = chain_check(w.c_str(), stages, c)) return rc;
    if (M == 0) return GPT_OK;
    const size_t D = c.v[K - 1].p.D;
    bool finite = all_finite(y, (size_t)M * D) && (!x0 || all_finite(x0, (size_t)M * D)) && std::isfinite(rtol) && std::isfinite(std_offset);
    for (int k = 0; k < K && finite; ++k) finite = affine_finite(c.g[k], D) && std::isfinite(c.scale[k]);
    if (!finite) return fail(GPT_E_ARG, w + ": y / x0 / the affine parts / rtol / std_offset contain NaN or infinity");
    gpt_handle* const owner = c.h[K - 1];
    CallResources* const res = call_resources(owner, CALL_CHAIN, CALL_EVENTS);
    if (!res) return GPT_E_HIP;
    ChunkStreams q;
    if (int rc = handle_copy_stream(owner, !one_chunk(M), &q)) return rc;
    if (int rc = upload_affine(*res, CHAIN_MAX, c.g, K, D, q.s)) return rc;
    // only what the caller asked for is staged and crosses the bus; the rest of what a later launch reads stays in the owner's
    // scratch.  A per-stage array is K planes: stage j's rows start at j * M rows on the host and at j * m rows in a chunk's image
    StagedArray table[CH_COUNT];
    for (int k = 0; k < CH_COUNT; ++k) table[k] = StagedArray{c.arr[k], row_bytes(k, D), k < CH_INPUTS, k >= CH_FIRST_STAGE ? K : 1};
    return run_chunked(res->st, q, table, M, [&](void* const* dev, int64_t m) {
        ChainCall d = c;
        d.M = m;
        for (int k = 0; k < K; ++k) d.g[k] = affine_slot(res->affine, k);
        std::copy(dev, dev + CH_COUNT, d.arr);
        return chain_dev(d);
    });
}
