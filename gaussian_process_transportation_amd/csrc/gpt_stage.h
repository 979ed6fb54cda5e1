// What the host entry points that work on handles share (internal header; plain C++, it also compiles under g++ against
// host_stub/, the sanitizer builds): the chunked, double-buffered staging of a host-pointer call (gpt_predict_all,
// gpt_transport_policy, gpt_pullback_policy, gpt_pullback_chain, gpt_rollout_policy, gpt_rollout_stabilised), the device image of a call's affine parts, the "caller's array
// or the handle's scratch" table, the one model check of the D <= 3 calls, and the three accessors through which
// gpt_transport_host.hip and gpt_chain_host.hip reach a handle (gpt_api.hip owns the type and defines them).
#pragma once
#include "gpt_call.h"

#include <algorithm>
#include <cstring>

struct gpt_handle;

namespace gpt {

constexpr int64_t HOST_CHUNK = 1 << 17;  // queries per chunk of a host-pointer call (two chunks in flight)
constexpr int STAGE_ARRAYS = 18;         // the longest array table (gpt_pullback_chain's)
constexpr int AFFINE_DOUBLES = 24;       // device image of one affine part: R (9) | R_jac (9) | c_src (3) | c_dst (3)
constexpr int AFFINE_SLOTS = 4;          // affine parts per call (the stages of a chain)
constexpr int CALL_SCRATCH = 6;          // most arrays a later launch of one call reads and the caller may not have asked for
constexpr int CALL_EVENTS = 2 * AFFINE_SLOTS + 1;

// ---- chunked staging
// One set of device images, one buffer per array of a call's table; grow-only, only what a call asks for is ever allocated.
struct StagingSet { DevBuf<unsigned char> buf[STAGE_ARRAYS]; };

// One array of a host-pointer call.  planes > 1: a (planes, M, ...) plane-major array, whose chunk image is (planes, m, ...) —
// every plane goes to its own place in the caller's array (dvar's D coordinates, the chain's K stages).
struct StagedArray {
    void* host;                          // the caller's array (only read when `input`), or null: neither staged nor copied
    size_t row_bytes;                    // per query (and plane)
    bool input;                          // travels to the device before the chunk computes, else from it afterwards
    int planes;
};

// The compute stream of a call; `copy` (with its two event pairs) is the handle's copy stream, null while no call of more than
// one chunk has created it.  handle_copy_stream() fills it.
struct ChunkStreams {
    hipStream_t s = nullptr, copy = nullptr;
    hipEvent_t ev_done[2] = {}, ev_copied[2] = {};   // chunk computed / chunk's outputs copied out, per staging set
};
inline bool one_chunk(int64_t M, int64_t chunk = HOST_CHUNK) { return M <= chunk; }

// Takes M > 0 queries through `compute(device pointers by table index, m)`, `chunk` (HOST_CHUNK unless a call's rows are long:
// gpt_rollout_policy) at a time.  One chunk (the reference's own
// batch sizes): inputs in, compute, outputs out, all in q.s — no second stream, no events.  Several chunks: chunk i computes on
// q.s in staging set i & 1 and its outputs leave on q.copy while chunk i + 1, enqueued before chunk i's host-blocking copies,
// computes; set b is reused only after ev_copied[b].  Returns after both streams have drained.  An input is one plane (no call
// has a plane-major input; its `planes` is not looked at).
template <int N, class Compute>
int run_chunked(StagingSet (&st)[2], const ChunkStreams& q, const StagedArray (&arr)[N], int64_t M, Compute&& compute,
                const int64_t chunk = HOST_CHUNK) {
    static_assert(N <= STAGE_ARRAYS, "a staging set has STAGE_ARRAYS buffers");
    constexpr int n = N;
    const int64_t cap = M < chunk ? M : chunk;
    const int64_t nchunks = (M + cap - 1) / cap;
    const bool single = nchunks == 1;
    hipStream_t s = q.s, cs = single ? q.s : q.copy;
    for (int b = 0; b < (single ? 1 : 2); ++b)
        for (int k = 0; k < n; ++k)
            if (arr[k].host) CALLCHK(reserve(st[b].buf[k], (size_t)cap * arr[k].row_bytes * arr[k].planes, s, q.copy));
    auto enqueue = [&](int64_t i) -> int {
        const int b = (int)(i & 1);
        const int64_t off = i * cap, m = (M - off) < cap ? (M - off) : cap;
        if (i >= 2) CALLCHK(hipStreamWaitEvent(s, q.ev_copied[b], 0));          // set b is free again
        void* dev[N];
        for (int k = 0; k < n; ++k) dev[k] = arr[k].host ? st[b].buf[k].p : nullptr;
        for (int k = 0; k < n; ++k)
            if (arr[k].host && arr[k].input)
                CALLCHK(hipMemcpyAsync(dev[k], static_cast<const unsigned char*>(arr[k].host) + (size_t)off * arr[k].row_bytes,
                                       (size_t)m * arr[k].row_bytes, hipMemcpyHostToDevice, s));
        if (int rc = compute(dev, m)) return rc;
        if (!single) CALLCHK(hipEventRecord(q.ev_done[b], s));
        return GPT_OK;
    };
    auto copy_out = [&](int64_t i) -> int {
        const int b = (int)(i & 1);
        const int64_t off = i * cap, m = (M - off) < cap ? (M - off) : cap;
        if (!single) CALLCHK(hipStreamWaitEvent(cs, q.ev_done[b], 0));
        for (int k = 0; k < n; ++k) {
            if (!arr[k].host || arr[k].input) continue;
            const size_t rb = arr[k].row_bytes;
            for (int j = 0; j < arr[k].planes; ++j)    // plane j: at j * M rows on the host, at j * m rows in the chunk's image
                CALLCHK(hipMemcpyAsync(static_cast<unsigned char*>(arr[k].host) + ((size_t)j * M + off) * rb, st[b].buf[k] + (size_t)j * m * rb,
                                       (size_t)m * rb, hipMemcpyDeviceToHost, cs));
        }
        if (!single) CALLCHK(hipEventRecord(q.ev_copied[b], cs));
        return GPT_OK;
    };
    if (int rc = enqueue(0)) return rc;
    for (int64_t i = 0; i < nchunks; ++i) {
        if (i + 1 < nchunks) { if (int rc = enqueue(i + 1)) return rc; }   // queued before chunk i's (host-blocking) copies
        if (int rc = copy_out(i)) return rc;
    }
    if (!single) CALLCHK(hipStreamSynchronize(cs));
    CALLCHK(hipStreamSynchronize(s));
    return GPT_OK;
}

// ---- a call's affine parts and scratch
struct AffinePart { const double *R, *R_jac, *c_src, *c_dst; };     // (D,D), (D,D), (D), (D)
inline AffinePart affine_slot(const double* image, int k) {
    const double* q = image + k * AFFINE_DOUBLES;
    return {q, q + 9, q + 18, q + 21};
}
inline bool affine_finite(const AffinePart& a, size_t D) {
    return all_finite(a.R, D * D) && all_finite(a.R_jac, D * D) && all_finite(a.c_src, D) && all_finite(a.c_dst, D);
}

// What a call family keeps on a handle between calls, created on first use (call_resources), each buffer grow-only.
struct CallResources {
    DevBuf<double> scratch[CALL_SCRATCH];    // what a later launch reads and the caller did not ask for
    StagingSet st[2];                        // of the chunked host call
    DevBuf<unsigned char> image;             // of gpt_inverse_map, which is not chunked: all its arrays carved from one buffer
    DevBuf<double> affine;                   // `slots` affine parts of the host call
    double affine_host[AFFINE_SLOTS * AFFINE_DOUBLES] = {};     // a member: the source of an asynchronous copy
    Event ev[CALL_EVENTS];                   // hand-over between the handles' streams
};

// `n` host affine parts into the first n of `slots` slots of r.affine (zero elsewhere), on s.
inline int upload_affine(CallResources& r, int slots, const AffinePart* parts, int n, size_t D, hipStream_t s) {
    const size_t doubles = (size_t)slots * AFFINE_DOUBLES;
    CALLCHK(reserve(r.affine, doubles * sizeof(double), s));
    double* ah = r.affine_host;
    CALLCHK(hipStreamSynchronize(s));          // (a copy out of it that an aborted call left in flight)
    std::fill(ah, ah + doubles, 0.0);
    for (int k = 0; k < n; ++k) {
        double* q = ah + k * AFFINE_DOUBLES;
        memcpy(q, parts[k].R, D * D * sizeof(double)); memcpy(q + 9, parts[k].R_jac, D * D * sizeof(double));
        memcpy(q + 18, parts[k].c_src, D * sizeof(double)); memcpy(q + 21, parts[k].c_dst, D * sizeof(double));
    }
    CALLCHK(hipMemcpyAsync(r.affine, ah, doubles * sizeof(double), hipMemcpyHostToDevice, s));
    return GPT_OK;
}

// An intermediate array of a call: table index, whether a launch of this call reads it, doubles per query.
struct MidArray { int which; bool need; size_t per; };
// at[k]: the caller's array when there is one, else (when needed) the scratch buffer, made large enough for M queries.
template <int N> int resolve_scratch(CallResources& r, void* const* u, const MidArray (&mid)[N], int64_t M, hipStream_t s, double* (&at)[N]) {
    static_assert(N <= CALL_SCRATCH, "scratch buffers of a call family");
    for (int k = 0; k < N; ++k) {
        at[k] = static_cast<double*>(u[mid[k].which]);
        if (mid[k].need && !at[k]) {
            CALLCHK(reserve(r.scratch[k], (size_t)M * mid[k].per * sizeof(double), s));
            at[k] = r.scratch[k];
        }
    }
    return GPT_OK;
}

// ---- a handle as the host units see it
struct ModelView {
    bool committed = false, matern_derivatives = false;
    int device = 0;
    hipStream_t stream = nullptr;
    KernelParams p{};
    const double *Xs = nullptr, *A4 = nullptr;      // scaled sources and alpha rows of the blob (fp64 models)
    const double* Wf = nullptr;                     // and its inverse factor in fragment order (fp64 models; k_pack_w)
};
enum { CALL_INVERSE = 0, CALL_TRANSPORT, CALL_PULLBACK, CALL_CHAIN, CALL_ROLLOUT, CALL_FAMILIES };

// The model of h as it is now (nothing is checked; h not null).
void model_view(gpt_handle* h, ModelView* v);
// The resources of call family `family` on h with their first `events` events created; h's device becomes the calling thread's.
// Null after a HIP failure (the error text is set).
CallResources* call_resources(gpt_handle* h, int family, int events);
// q->s = h's stream; h's copy stream and its event pairs as they are, or (create) created on first use.
int handle_copy_stream(gpt_handle* h, bool create, ChunkStreams* q);

// What a model of the D <= 3 calls must be, in the words of the call.  role: "" for a call's only model ("this model"), else
// the model's name in the call ("map": "the map model").  matern12 / matern: the refusals of a model whose derivatives the call
// needs and that has none / has them switched off; null when the model is only evaluated (any of the four kernels).
struct ModelCheck { const char *role, *what, *matern12, *matern; };
// the refusals of a map through which a policy is pulled back (gpt_pullback_policy, every stage of gpt_pullback_chain)
constexpr const char* PULLBACK_MATERN12 =
    ": a Matern 1/2 (nu = 0.5) map is not differentiable at the training points: Newton has no Jacobian and the velocities nothing to "
    "be pushed through; use RBF, Matern 3/2 or Matern 5/2";
constexpr const char* PULLBACK_MATERN =
    ": the pull-back through a Matern map uses the analytic derivatives of its posterior; gpt_set_matern_derivatives(h_map, 1) enables them";
// a committed model of a space onto itself, D == O <= 3
inline int check_model_shape(gpt_handle* h, const std::string& w, const ModelCheck& c, ModelView* v) {
    const std::string r(c.role);
    if (!h) return fail(GPT_E_ARG, w + ": NULL handle" + (r.empty() ? "" : " (" + r + ")"));
    model_view(h, v);
    if (!v->committed) return fail(GPT_E_STATE, w + (r.empty() ? ": model is not fitted" : ": the " + r + " model is not fitted"));
    const KernelParams& p = v->p;
    if (p.D != p.O || p.D > 3)
        return fail(GPT_E_ARG, w + (r.empty() ? ": the " + std::string(c.what) + " needs a map of" : ": the " + r + " model must map") +
                                   " a space onto itself, D == O, with D <= 3 (this model: D = " + std::to_string(p.D) + ", O = " +
                                   std::to_string(p.O) + ")");
    return GPT_OK;
}
// fp64, single-task, and differentiable where the call needs derivatives
inline int check_model_kind(const ModelView& v, const std::string& w, const ModelCheck& c) {
    auto model = [&] { return c.role[0] ? "the " + std::string(c.role) + " model" : std::string("this model"); };
    const KernelParams& p = v.p;
    if (p.dtype != DT_F64) return fail(GPT_E_ARG, w + ": fp64 models only (" + model() + " was fitted with GPT_F32)");
    if (p.ntask != 1) return fail(GPT_E_ARG, w + ": single-task models only (" + model() + " is a multi-task gpt_fit_svgp model)");
    if (!c.matern12) return GPT_OK;
    if (p.ktype == GPT_KERNEL_MATERN12) return fail(GPT_E_ARG, w + c.matern12);
    if (p.ktype != GPT_KERNEL_RBF && !v.matern_derivatives) return fail(GPT_E_ARG, w + c.matern);
    return GPT_OK;
}
inline int check_model(gpt_handle* h, const std::string& w, const ModelCheck& c, ModelView* v) {
    if (int rc = check_model_shape(h, w, c, v)) return rc;
    return check_model_kind(*v, w, c);
}

}  // namespace gpt
