// What the rollout families share on the host (gpt_rollout_host.hip: the mean policy; gpt_rollout_stab_host.hip: the
// variance-stabilised one; gpt_rollout_sampled_host.hip: the sampled one): the refusals all state in the same words, the launches
// of one call enqueued back to back with the hand-over between the handles' streams, and the chunked staging of the host call.  A
// family brings its array table (its first arrays are the inputs, y0 and x0 ahead), the bytes of a row of each array, and its launcher.  Internal header, host code only; plain C++,
// it also compiles under g++ against host_stub/.  The resources of a call (CALL_ROLLOUT) are held by the handle of the LAST stage,
// or by the dynamics' when there is no stage; its events: ev[j] the j-th other stream has caught up, ev[2 CHAIN_MAX] the last
// launch is done.
#pragma once
#include "gpt_rollout.h"
#include "gpt_chain_check.h"

namespace gpt {

// the arguments of every entry point but its arrays
struct RolloutCallBase : ChainModels {
    int64_t M = 0, T = 0;
    double dt = 0.0, rtol = 0.0;
    int max_passes = 0;
};

// what every entry point refuses of the solver, the steps and the sizes, in the order of the header's list; required: y0, path,
// steps_done and status are all there
inline int rollout_check_args(const std::string& w, const RolloutCallBase& c, bool required) {
    if (int rc = chain_check_solver(w, c.rtol, c.max_passes)) return rc;
    if (c.T < 0) return fail(GPT_E_ARG, w + ": n_steps must be >= 0");
    if (!std::isfinite(c.dt) || c.dt == 0.0) return fail(GPT_E_ARG, w + ": dt must be finite and not zero");
    if (c.M < 0 || c.M >= ((int64_t)1 << 31)) return fail(GPT_E_ARG, w + ": M must be 0 .. 2^31 - 1");
    if (c.T >= ((int64_t)1 << 31) || c.M * (c.T + 1) >= ((int64_t)1 << 31))
        return fail(GPT_E_ARG, w + ": M (n_steps + 1), the rows of path, must be below 2^31");
    if (c.M > 0 && !required) return fail(GPT_E_ARG, w + ": y0, path, steps_done and status must not be NULL");
    return GPT_OK;
}

// Every pointer in device memory; enqueues the whole call, waits for nothing.  `a`: the kernel's arguments with the arrays already
// in place; the models, the sizes, the solver, `state` and the launch window are filled here.  launch(stream, D) enqueues one
// launch of the window a.t_begin .. a.t_end, at most `per` steps.
template <class Launch>
int rollout_enqueue(const RolloutCallBase& c, RolloutArgs& a, int per, Launch&& launch) {
    gpt_handle* const owner = c.owner();
    CallResources* const res = call_resources(owner, CALL_ROLLOUT, CALL_EVENTS);
    if (!res) return GPT_E_HIP;
    const Event *ev_in = res->ev, &ev_done = res->ev[2 * CHAIN_MAX];
    hipStream_t s = c.owner_view().stream;
    const size_t D = c.owner_view().p.D;
    const int T = (int)c.T;
    a.M = c.M; a.K = c.K;
    chain_kernel_models(c, a.st, a.dyn);
    a.rtol = c.rtol; a.max_passes = c.max_passes; a.dt = c.dt; a.T = T;
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
        launch(s, (int)D);
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

// The host entry of a family after its checks, M > 0: the finite inputs, then the trajectories through the device in chunks of about
// ROLLOUT_CHUNK_ROWS path rows, whatever T is.  Call: a RolloutCallBase with `void* arr[N]`, arr[0] = y0, arr[1] = x0 the inputs;
// row_bytes(k, D, T): bytes per trajectory of array k; dev(call): the family's device entry on a chunk.  n_inputs: the first so many
// arrays travel to the device (a family checks its inputs beyond y0 and x0 itself); max_chunk > 0: trajectories a chunk may hold at
// most, where a family's device scratch sets a limit of its own.
template <int N, class Call, class RowBytes, class Dev>
int rollout_host_chunks(const std::string& w, const Call& c, RowBytes&& row_bytes, Dev&& dev, const int n_inputs = RO_INPUTS,
                        const int64_t max_chunk = 0) {
    const size_t D = c.owner_view().p.D, T = (size_t)c.T;
    const double *y0 = static_cast<const double*>(c.arr[0]), *x0 = static_cast<const double*>(c.arr[1]);
    bool finite = all_finite(y0, (size_t)c.M * D) && (!x0 || all_finite(x0, (size_t)c.M * D)) && std::isfinite(c.rtol);
    for (int k = 0; k < c.K && finite; ++k) finite = affine_finite(c.g[k], D) && std::isfinite(c.scale[k]);
    if (!finite) return fail(GPT_E_ARG, w + ": y0 / x0 / the affine parts / rtol contain NaN or infinity");
    gpt_handle* const owner = c.owner();
    CallResources* const res = call_resources(owner, CALL_ROLLOUT, CALL_EVENTS);
    if (!res) return GPT_E_HIP;
    int64_t chunk = std::max<int64_t>(1, ROLLOUT_CHUNK_ROWS / (c.T + 1));
    if (max_chunk > 0) chunk = std::min(chunk, max_chunk);
    ChunkStreams q;
    if (int rc = handle_copy_stream(owner, !one_chunk(c.M, chunk), &q)) return rc;
    if (int rc = upload_affine(*res, CHAIN_MAX, c.g, c.K, D, q.s)) return rc;
    // only what the caller asked for is staged and crosses the bus (with T = 0 the per-step arrays have no rows)
    StagedArray table[N];
    for (int k = 0; k < N; ++k) {
        const size_t rb = row_bytes(k, D, T);
        table[k] = StagedArray{rb ? c.arr[k] : nullptr, rb, k < n_inputs, 1};
    }
    return run_chunked(res->st, q, table, c.M, [&](void* const* dev_arr, int64_t m) {
        Call d = c;
        d.M = m;
        for (int k = 0; k < c.K; ++k) d.g[k] = affine_slot(res->affine, k);
        std::copy(dev_arr, dev_arr + N, d.arr);
        return dev(d);
    }, chunk);
}

}  // namespace gpt
