// What the entry points that take a gpt_chain_stage array share on the host (gpt_chain_host.hip, gpt_rollout_host.hip): the
// handles and affine parts of a call, the refusals both state in the same words, and the kernels' view of the models  (internal
// header; plain C++, it also compiles under g++ against host_stub/).
#pragma once
#include "gpt_chain.h"
#include "gpt_stage.h"

namespace gpt {

static_assert(CHAIN_MAX == AFFINE_SLOTS, "the chain is the call with the most affine parts (gpt_stage.h)");

// the maps and the dynamics of a call (host or device pointers alike in g)
struct ChainModels {
    int K = 0;
    gpt_handle* h[CHAIN_MAX] = {};
    gpt_handle* h_dyn = nullptr;
    ModelView v[CHAIN_MAX], v_dyn;
    AffinePart g[CHAIN_MAX] = {};
    double scale[CHAIN_MAX] = {};
    // the model whose handle owns the call's stream, scratch and staging: the last stage, or the dynamics of a call without maps
    gpt_handle* owner() const { return K ? h[K - 1] : h_dyn; }
    const ModelView& owner_view() const { return K ? v[K - 1] : v_dyn; }
};

// what the wave-level passes read of a model
inline ChainModel chain_model(const ModelView& v) {
    ChainModel m{};
    m.N = v.p.N; m.ktype = v.p.ktype; m.lnc = v.p.lnc;
    for (int d = 0; d < 3; ++d) m.inv_ls[d] = v.p.inv_ls[d];
    m.Xs = v.Xs; m.A4 = v.A4;
    return m;
}

// the stages and the dynamics as a kernel's arguments
inline void chain_kernel_models(const ChainModels& c, ChainStage (&st)[CHAIN_MAX], ChainModel& dyn) {
    for (int k = 0; k < c.K; ++k) {
        st[k].m = chain_model(c.v[k]);
        st[k].R = c.g[k].R; st[k].c_src = c.g[k].c_src; st[k].c_dst = c.g[k].c_dst; st[k].R_jac = c.g[k].R_jac; st[k].scale = c.scale[k];
    }
    dyn = chain_model(c.v_dyn);
}

// What is refused of K (c.K, at least K_min), the stages array, the handles and their models, in the order of the header's list;
// fills the views.
inline int chain_check_models(const std::string& w, const gpt_chain_stage* stages, int K_min, ChainModels& c) {
    if (c.K < K_min || c.K > CHAIN_MAX)
        return fail(GPT_E_ARG, w + ": K must be " + std::to_string(K_min) + " .. " + std::to_string(CHAIN_MAX) + " (GPT_CHAIN_MAX) stages, got " +
                                   std::to_string(c.K));
    if (c.K > 0 && !stages) return fail(GPT_E_ARG, w + ": stages must not be NULL");
    for (int k = 0; k < c.K; ++k) {
        const std::string role = "stage " + std::to_string(k) + " map";
        c.h[k] = stages[k].h; c.g[k] = AffinePart{stages[k].R, stages[k].R_jac, stages[k].c_src, stages[k].c_dst};
        c.scale[k] = stages[k].scale;
        if (!c.h[k]) return fail(GPT_E_ARG, w + ": NULL handle (" + role + ")");
        if (!c.g[k].R || !c.g[k].c_src || !c.g[k].c_dst || !c.g[k].R_jac)
            return fail(GPT_E_ARG, w + ": R, c_src, c_dst and R_jac must not be NULL (stage " + std::to_string(k) + ")");
    }
    if (!c.h_dyn) return fail(GPT_E_ARG, w + ": NULL handle (dynamics)");
    for (int k = 0; k < c.K; ++k) {
        for (int j = 0; j < k; ++j)
            if (c.h[j] == c.h[k])
                return fail(GPT_E_ARG, w + ": stages " + std::to_string(j) + " and " + std::to_string(k) + " are the same handle; every stage is a model of its own");
        if (c.h[k] == c.h_dyn)
            return fail(GPT_E_ARG, w + ": stage " + std::to_string(k) + " and h_dyn are the same handle; the maps and the dynamics are separate models");
    }
    for (int k = 0; k < c.K; ++k) {
        const std::string role = "stage " + std::to_string(k) + " map";
        if (int rc = check_model(c.h[k], w, ModelCheck{role.c_str(), "", PULLBACK_MATERN12, PULLBACK_MATERN}, &c.v[k])) return rc;
    }
    if (int rc = check_model(c.h_dyn, w, ModelCheck{"dynamics", "", nullptr, nullptr}, &c.v_dyn)) return rc;
    for (int k = 0; k < c.K; ++k) {
        const ModelView& last = c.v[c.K - 1];
        const ModelView& v = k + 1 < c.K ? c.v[k] : c.v_dyn;
        const std::string name = k + 1 < c.K ? "stage " + std::to_string(k) : std::string("the dynamics");
        if (v.device != last.device)
            return fail(GPT_E_ARG, w + ": the models live on different devices (stage " + std::to_string(c.K - 1) + ": " + std::to_string(last.device) +
                                       ", " + name + ": " + std::to_string(v.device) + "); gpt_factor_copy brings one to the other's");
        if (v.p.D != last.p.D)
            return fail(GPT_E_ARG, w + ": every map and the dynamics must share one space (stage " + std::to_string(c.K - 1) + ": D = " +
                                       std::to_string(last.p.D) + ", " + name + ": D = " + std::to_string(v.p.D) + ")");
    }
    return GPT_OK;
}

inline int chain_check_solver(const std::string& w, double rtol, int max_passes) {
    if (!(rtol > 0.0)) return fail(GPT_E_ARG, w + ": rtol must be > 0");
    if (max_passes < 1) return fail(GPT_E_ARG, w + ": max_passes must be >= 1");
    return GPT_OK;
}

// The other handles of a call, stages 0 .. K-2 and the dynamics (none when K = 0): what their streams have enqueued so far (a
// fit, a gpt_factor_commit) comes before what `s` gets from here on.  Fills other[0 .. K-1]; ev: K events.
inline int chain_wait_for_others(const ChainModels& c, hipStream_t s, const Event* ev, hipStream_t (&other)[CHAIN_MAX]) {
    for (int j = 0; j < c.K; ++j) other[j] = j + 1 < c.K ? c.v[j].stream : c.v_dyn.stream;
    for (int j = 0; j < c.K; ++j) {
        CALLCHK(hipEventRecord(ev[j], other[j]));
        CALLCHK(hipStreamWaitEvent(s, ev[j], 0));
    }
    return GPT_OK;
}

}  // namespace gpt
