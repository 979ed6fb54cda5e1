// gpt_inverse_map, gpt_transport_policy, gpt_pullback_policy and their _dev forms (include/gpt_hip.h): argument checks, the
// scratch between the launches, the hand-over between the two handles' streams of the pull-back, and the staging of the host
// calls.  Host code only (the kernels: gpt_inverse.hip, gpt_transport.hip, gpt_pullback.hip, reached through their launchers;
// the handles: through the accessors of gpt_stage.h), so it also compiles under g++ against host_stub/ and runs under the
// sanitizers (make host-asan, make host-oneshot-asan).  The layout of gpt_chain_host.hip.
#include "gpt_stage.h"
#include "gpt_transport.h"
#include "gpt_pullback.h"

using namespace gpt;

static_assert(GPT_INV_CONVERGED == INV_CONVERGED && GPT_INV_MAX_PASSES == INV_MAX_PASSES && GPT_INV_SINGULAR == INV_SINGULAR &&
              GPT_INV_STALLED == INV_STALLED, "status codes of the header and of the kernel");

namespace {

// arrays of gpt_transport_policy, in the order of its arguments: inputs, outputs, the posterior the epilogue consumed
enum { TP_POS = 0, TP_VEL, TP_ORI, TP_POS_ROT, TP_POS_OUT, TP_VAR, TP_VEL_OUT, TP_VEL_VAR, TP_DET_VEL, TP_ORI_OUT, TP_DET_ORI, TP_ORI_GAP,
       TP_MEAN, TP_J, TP_JVAR, TP_J_ORI, TP_COUNT };
constexpr int TP_INPUTS = 3;             // TP_POS .. TP_ORI travel to the device, the rest from it
// arrays of gpt_pullback_policy, in the order of its arguments (passes and status hold ints, the rest doubles)
enum { PB_Y = 0, PB_X0, PB_X, PB_VEL, PB_F, PB_DET, PB_RES, PB_PASSES, PB_STATUS, PB_VAR_DYN, PB_MAP_VAR, PB_VVAR_MAP, PB_VVAR_DYN,
       PB_Z, PB_A, PB_JVAR, PB_COUNT };
constexpr int PB_INPUTS = 2;             // PB_Y, PB_X0 travel to the device, the rest from it

const ModelCheck INVERSE_MODEL = {
    "", "inverse",
    ": Matern 1/2 (nu = 0.5) is not differentiable at the training points: Newton has no Jacobian; use RBF, Matern 3/2 or Matern 5/2",
    ": the inverse of a Matern model uses the analytic derivatives of its posterior; gpt_set_matern_derivatives(h, 1) enables them"};
const ModelCheck TRANSPORT_MODEL = {
    "", "transport",
    ": Matern 1/2 (nu = 0.5) is not differentiable at the training points: the map has no Jacobian to push velocities and orientations "
    "through; use RBF, Matern 3/2 or Matern 5/2",
    ": the transport through a Matern model uses the analytic derivatives of its posterior; gpt_set_matern_derivatives(h, 1) enables them"};

// what both inverse entry points refuse, in the order of the header's list
int inverse_check(gpt_handle* h, const char* who, const double* Y, int64_t M, double rtol, int max_passes, const double* Z, const int* status,
                  ModelView* v) {
    const std::string w(who);
    if (int rc = check_model(h, w, INVERSE_MODEL, v)) return rc;
    if (!(rtol > 0.0)) return fail(GPT_E_ARG, w + ": rtol must be > 0");
    if (max_passes < 1) return fail(GPT_E_ARG, w + ": max_passes must be >= 1");
    if (M < 0 || M >= ((int64_t)1 << 31)) return fail(GPT_E_ARG, w + ": M must be 0 .. 2^31 - 1");
    if (M > 0 && (!Y || !Z || !status)) return fail(GPT_E_ARG, w + ": Y, Z and status must not be NULL");
    return GPT_OK;
}

int inverse_dev(const ModelView& v, const InverseArgs& a) {
    CALLCHK(hipSetDevice(v.device));
    launch_inverse_newton(v.stream, v.p, v.Xs, v.A4, a);
    CALLCHK(hipGetLastError());
    return GPT_OK;
}

}  // namespace

extern "C" int gpt_inverse_map_dev(gpt_handle* h, const double* Y, const double* Z0, int64_t M, double rtol, int max_passes, double* Z,
                                   double* residual, double* det, int* passes, int* status) {
    ModelView v;
    if (int rc = inverse_check(h, "gpt_inverse_map_dev", Y, M, rtol, max_passes, Z, status, &v)) return rc;
    if (M == 0) return GPT_OK;
    return inverse_dev(v, InverseArgs{Y, Z0, M, rtol, max_passes, Z, residual, det, passes, status});
}

extern "C" int gpt_inverse_map(gpt_handle* h, const double* Y, const double* Z0, int64_t M, double rtol, int max_passes, double* Z,
                               double* residual, double* det, int* passes, int* status) {
    ModelView v;
    if (int rc = inverse_check(h, "gpt_inverse_map", Y, M, rtol, max_passes, Z, status, &v)) return rc;
    if (M == 0) return GPT_OK;
    const size_t D = v.p.D, nv = (size_t)M * D;
    if (!all_finite(Y, nv) || (Z0 && !all_finite(Z0, nv))) return fail(GPT_E_ARG, "gpt_inverse_map: Y / Z0 contain NaN or infinity");
    CallResources* const res = call_resources(h, CALL_INVERSE, 0);
    if (!res) return GPT_E_HIP;
    hipStream_t s = v.stream;
    // one grow-only image, not chunked: [Y | Z0 | Z | residual | det | passes | status]
    const size_t bv = nv * sizeof(double), bs = (size_t)M * sizeof(double), bi = ((size_t)M * sizeof(int) + 15) / 16 * 16;
    CALLCHK(reserve(res->image, 3 * bv + 2 * bs + 2 * bi, s));
    unsigned char* const b = res->image;
    double *dY = reinterpret_cast<double*>(b), *dZ0 = reinterpret_cast<double*>(b + bv), *dZ = reinterpret_cast<double*>(b + 2 * bv),
           *dres = reinterpret_cast<double*>(b + 3 * bv), *ddet = reinterpret_cast<double*>(b + 3 * bv + bs);
    int *dpass = reinterpret_cast<int*>(b + 3 * bv + 2 * bs), *dstat = reinterpret_cast<int*>(b + 3 * bv + 2 * bs + bi);
    CALLCHK(hipMemcpyAsync(dY, Y, bv, hipMemcpyHostToDevice, s));
    if (Z0) CALLCHK(hipMemcpyAsync(dZ0, Z0, bv, hipMemcpyHostToDevice, s));
    if (int rc = inverse_dev(v, InverseArgs{dY, Z0 ? dZ0 : nullptr, M, rtol, max_passes, dZ, residual ? dres : nullptr, det ? ddet : nullptr,
                                            passes ? dpass : nullptr, dstat}))
        return rc;
    CALLCHK(hipMemcpyAsync(Z, dZ, bv, hipMemcpyDeviceToHost, s));
    if (residual) CALLCHK(hipMemcpyAsync(residual, dres, bs, hipMemcpyDeviceToHost, s));
    if (det) CALLCHK(hipMemcpyAsync(det, ddet, bs, hipMemcpyDeviceToHost, s));
    if (passes) CALLCHK(hipMemcpyAsync(passes, dpass, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, s));
    CALLCHK(hipMemcpyAsync(status, dstat, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, s));
    CALLCHK(hipStreamSynchronize(s));
    return GPT_OK;
}

// ---- transport of positions, velocities and orientations: affine part, posterior, push-forward, all on the device
namespace {

// the arguments of both transport entry points (host or device pointers alike), arrays indexed by TP_*
struct TransportCall {
    gpt_handle* h = nullptr;
    ModelView v;
    int64_t M = 0;
    double scale = 1.0;
    AffinePart g{};
    void* arr[TP_COUNT] = {};            // doubles all; the inputs TP_POS .. TP_ORI are only read
};

// what both entry points refuse, in the order of the header's list; fills the view
int transport_check(const char* who, TransportCall& c) {
    const std::string w(who);
    if (int rc = check_model_shape(c.h, w, TRANSPORT_MODEL, &c.v)) return rc;
    const int D = c.v.p.D;
    if ((c.arr[TP_ORI] || c.arr[TP_ORI_OUT] || c.arr[TP_ORI_GAP]) && D != 3)
        return fail(GPT_E_ARG, w + ": orientations (ori, ori_out, ori_gap) need D == 3: the rotation closest to a " + std::to_string(D) +
                                   " x " + std::to_string(D) + " Jacobian is no quaternion");
    if (int rc = check_model_kind(c.v, w, TRANSPORT_MODEL)) return rc;
    if (c.M < 0 || c.M >= ((int64_t)1 << 31)) return fail(GPT_E_ARG, w + ": M must be 0 .. 2^31 - 1");
    if ((c.arr[TP_VEL_OUT] || c.arr[TP_VEL_VAR]) && !c.arr[TP_VEL])
        return fail(GPT_E_ARG, w + ": vel_out and vel_var need vel (the velocities to push forward)");
    if (c.arr[TP_ORI_OUT] && !c.arr[TP_ORI]) return fail(GPT_E_ARG, w + ": ori_out needs ori (the orientations to rotate)");
    if (c.M > 0 && (!c.arr[TP_POS] || !c.arr[TP_POS_OUT] || !c.g.R || !c.g.c_src || !c.g.c_dst || !c.g.R_jac))
        return fail(GPT_E_ARG, w + ": pos, pos_out, R, c_src, c_dst and R_jac must not be NULL");
    return GPT_OK;
}

// every pointer of `c` in device memory; enqueues the whole call, waits for nothing
int transport_dev(const TransportCall& c) {
    CallResources* const res = call_resources(c.h, CALL_TRANSPORT, 0);
    if (!res) return GPT_E_HIP;
    hipStream_t s = c.v.stream;
    const int64_t M = c.M;
    const size_t D = c.v.p.D;
    void* const* u = c.arr;
    // which posterior quantities the outputs asked for consume
    const bool need_J = u[TP_VEL_OUT] || u[TP_DET_VEL] || u[TP_J];
    const bool need_Jvar = u[TP_VEL_VAR] || u[TP_JVAR];
    const bool need_J_ori = u[TP_ORI_OUT] || u[TP_DET_ORI] || u[TP_ORI_GAP] || u[TP_J_ORI];
    const MidArray mid[5] = {{TP_POS_ROT, true, D}, {TP_MEAN, true, D}, {TP_J, need_J, D * D}, {TP_JVAR, need_Jvar, D}, {TP_J_ORI, need_J_ori, D * D}};
    double* at[5];
    if (int rc = resolve_scratch(*res, u, mid, M, s, at)) return rc;
    auto dbl = [&](int k) { return static_cast<double*>(u[k]); };
    TransportArgs a{};
    a.M = M; a.scale = c.scale; a.R = c.g.R; a.c_src = c.g.c_src; a.c_dst = c.g.c_dst; a.R_jac = c.g.R_jac;
    a.pos = dbl(TP_POS); a.vel = dbl(TP_VEL); a.ori = dbl(TP_ORI);
    a.pos_rot = at[0]; a.mean = at[1]; a.J = at[2]; a.Jvar = at[3]; a.J_ori = at[4];
    a.pos_out = dbl(TP_POS_OUT); a.vel_out = dbl(TP_VEL_OUT); a.vel_var = dbl(TP_VEL_VAR); a.det_vel = dbl(TP_DET_VEL);
    a.ori_out = dbl(TP_ORI_OUT); a.det_ori = dbl(TP_DET_ORI); a.ori_gap = dbl(TP_ORI_GAP);
    launch_transport_affine(s, (int)D, a);
    // the Jacobian at the un-rotated positions (the reference's transport_orientation), then the posterior at gamma(pos): the
    // launches, query image and choice of variance path of gpt_predict_all_dev itself
    if (need_J_ori) launch_mean_jac(s, c.v.p, c.v.Xs, c.v.A4, a.pos, M, nullptr, at[4]);
    if (int rc = gpt_predict_all_dev(c.h, a.pos_rot, M, at[1], u[TP_VAR], at[2], at[3], nullptr)) return rc;
    launch_transport_push(s, (int)D, a);
    CALLCHK(hipGetLastError());
    return GPT_OK;
}

}  // namespace

#define TRANSPORT_CALL(c)                                                                                                          \
    TransportCall c;                                                                                                               \
    c.h = h; c.M = M; c.scale = scale; c.g = AffinePart{R, R_jac, c_src, c_dst};                                                   \
    {                                                                                                                              \
        const void* const all[TP_COUNT] = {pos, vel, ori, pos_rot, pos_out, var, vel_out, vel_var, det_vel, ori_out, det_ori, ori_gap, \
                                           post_mean, post_J, post_Jvar, post_J_ori};                                             \
        for (int k = 0; k < TP_COUNT; ++k) c.arr[k] = const_cast<void*>(all[k]);                                                   \
    }

extern "C" int gpt_transport_policy_dev(gpt_handle* h, const double* pos, int64_t M, const double* R, const double* c_src,
                                        const double* c_dst, double scale, const double* R_jac, const double* vel, const double* ori,
                                        double* pos_rot, double* pos_out, double* var, double* vel_out, double* vel_var, double* det_vel,
                                        double* ori_out, double* det_ori, double* ori_gap, double* post_mean, double* post_J,
                                        double* post_Jvar, double* post_J_ori) {
    TRANSPORT_CALL(c);
    if (int rc = transport_check("gpt_transport_policy_dev", c)) return rc;
    if (M == 0) return GPT_OK;
    return transport_dev(c);
}

extern "C" int gpt_transport_policy(gpt_handle* h, const double* pos, int64_t M, const double* R, const double* c_src, const double* c_dst,
                                    double scale, const double* R_jac, const double* vel, const double* ori, double* pos_rot,
                                    double* pos_out, double* var, double* vel_out, double* vel_var, double* det_vel, double* ori_out,
                                    double* det_ori, double* ori_gap, double* post_mean, double* post_J, double* post_Jvar,
                                    double* post_J_ori) {
    TRANSPORT_CALL(c);
    if (int rc = transport_check("gpt_transport_policy", c)) return rc;
    if (M == 0) return GPT_OK;
    const size_t D = c.v.p.D, W = sizeof(double);
    if (!all_finite(pos, (size_t)M * D) || (vel && !all_finite(vel, (size_t)M * D)) || (ori && !all_finite(ori, (size_t)M * 4)) ||
        !affine_finite(c.g, D) || !std::isfinite(scale))
        return fail(GPT_E_ARG, "gpt_transport_policy: pos / vel / ori / the affine part contain NaN or infinity");
    CallResources* const res = call_resources(h, CALL_TRANSPORT, 0);
    if (!res) return GPT_E_HIP;
    ChunkStreams q;
    if (int rc = handle_copy_stream(h, !one_chunk(M), &q)) return rc;
    if (int rc = upload_affine(*res, 1, &c.g, 1, D, q.s)) return rc;
    // only what the caller asked for is staged and crosses the bus; the rest of what the epilogue reads stays in the handle's scratch
    const size_t per[TP_COUNT] = {D, D, 4, D, D, 1, D, 1, 1, 4, 1, 1, D, D * D, D, D * D};       // doubles per query, by TP_*
    StagedArray table[TP_COUNT];
    for (int k = 0; k < TP_COUNT; ++k) table[k] = StagedArray{c.arr[k], per[k] * W, k < TP_INPUTS, 1};
    return run_chunked(res->st, q, table, M, [&](void* const* dev, int64_t m) {
        TransportCall d = c;
        d.M = m; d.g = affine_slot(res->affine, 0);
        std::copy(dev, dev + TP_COUNT, d.arr);
        return transport_dev(d);
    });
}

// ---- the transported policy at target-space points: Newton, affine inverse, dynamics mean and push-forward in one launch on the
// map handle's stream; the two variance launches (unchanged), each on its own handle's stream; a one-thread-per-query epilogue
namespace {

const ModelCheck PULLBACK_MAP = {"map", "", PULLBACK_MATERN12, PULLBACK_MATERN};
const ModelCheck PULLBACK_DYNAMICS = {"dynamics", "", nullptr, nullptr};      // only evaluated: any of the four kernels

// the arguments of both pullback entry points (host or device pointers alike), arrays indexed by PB_*
struct PullbackCall {
    gpt_handle *hm = nullptr, *hd = nullptr;
    ModelView vm, vd;
    int64_t M = 0;
    double scale = 1.0, rtol = 0.0, std_offset = 0.0;
    int max_passes = 0;
    AffinePart g{};
    void* arr[PB_COUNT] = {};            // (the inputs PB_Y, PB_X0 are only read)
};

// what both entry points refuse, in the order of the header's list; fills the views
int pullback_check(const char* who, PullbackCall& c) {
    const std::string w(who);
    if (int rc = check_model(c.hm, w, PULLBACK_MAP, &c.vm)) return rc;
    if (int rc = check_model(c.hd, w, PULLBACK_DYNAMICS, &c.vd)) return rc;
    if (c.hm == c.hd) return fail(GPT_E_ARG, w + ": h_map and h_dyn are the same handle; the map and the dynamics are two models");
    if (c.vm.device != c.vd.device)
        return fail(GPT_E_ARG, w + ": the two models live on different devices (map: " + std::to_string(c.vm.device) + ", dynamics: " +
                                   std::to_string(c.vd.device) + "); gpt_factor_copy brings one to the other's");
    if (c.vm.p.D != c.vd.p.D)
        return fail(GPT_E_ARG, w + ": the map and the dynamics must share one space (map: D = " + std::to_string(c.vm.p.D) +
                                   ", dynamics: D = " + std::to_string(c.vd.p.D) + ")");
    if (!(c.rtol > 0.0)) return fail(GPT_E_ARG, w + ": rtol must be > 0");
    if (c.max_passes < 1) return fail(GPT_E_ARG, w + ": max_passes must be >= 1");
    if (c.M < 0 || c.M >= ((int64_t)1 << 31)) return fail(GPT_E_ARG, w + ": M must be 0 .. 2^31 - 1");
    if (c.M > 0 && (!c.arr[PB_Y] || !c.arr[PB_VEL] || !c.arr[PB_STATUS] || !c.g.R || !c.g.c_src || !c.g.c_dst || !c.g.R_jac))
        return fail(GPT_E_ARG, w + ": y, vel, status, R, c_src, c_dst and R_jac must not be NULL");
    return GPT_OK;
}

// every pointer of `c` in device memory; enqueues the whole call, waits for nothing
int pullback_dev(const PullbackCall& c) {
    CallResources* const res = call_resources(c.hm, CALL_PULLBACK, 3);
    if (!res) return GPT_E_HIP;
    hipStream_t s = c.vm.stream, sd = c.vd.stream;
    const int64_t M = c.M;
    const size_t D = c.vm.p.D;
    void* const* u = c.arr;
    // which intermediate quantities the outputs asked for consume
    const bool need_var_dyn = u[PB_VAR_DYN] || u[PB_VVAR_DYN];
    const bool need_jvar = u[PB_JVAR] || u[PB_VVAR_MAP];
    const bool need_map = u[PB_MAP_VAR] || need_jvar;               // map_var and Jvar together: one pass of the 4-column launch
    const bool epilogue = u[PB_VVAR_MAP] || u[PB_VVAR_DYN];
    const MidArray mid[6] = {{PB_X, need_var_dyn, D}, {PB_Z, need_map, D}, {PB_F, epilogue, D}, {PB_A, u[PB_VVAR_DYN] != nullptr, D * D},
                             {PB_VAR_DYN, need_var_dyn, 1}, {PB_JVAR, need_jvar, D}};
    double* at[6];
    if (int rc = resolve_scratch(*res, u, mid, M, s, at)) return rc;
    PullbackArgs a{};
    a.M = M; a.scale = c.scale; a.R = c.g.R; a.c_src = c.g.c_src; a.c_dst = c.g.c_dst; a.R_jac = c.g.R_jac;
    a.Y = static_cast<const double*>(u[PB_Y]); a.X0 = static_cast<const double*>(u[PB_X0]);
    a.rtol = c.rtol; a.max_passes = c.max_passes; a.std_offset = c.std_offset;
    a.x = at[0]; a.z = at[1]; a.f = at[2]; a.A = at[3];
    a.vel = static_cast<double*>(u[PB_VEL]); a.det = static_cast<double*>(u[PB_DET]); a.residual = static_cast<double*>(u[PB_RES]);
    a.passes = static_cast<int*>(u[PB_PASSES]); a.status = static_cast<int*>(u[PB_STATUS]);
    a.var_dyn = at[4]; a.Jvar = at[5];
    a.vel_var_map = static_cast<double*>(u[PB_VVAR_MAP]); a.vel_var_dyn = static_cast<double*>(u[PB_VVAR_DYN]);
    // what the dynamics handle's stream has enqueued so far (its fit, a gpt_factor_commit) comes first
    CALLCHK(hipEventRecord(res->ev[0], sd));
    CALLCHK(hipStreamWaitEvent(s, res->ev[0], 0));
    launch_pullback_velocity(s, c.vm.p, c.vm.Xs, c.vm.A4, c.vd.p, c.vd.Xs, c.vd.A4, a);
    // the dynamics handle's stream goes on once x is there and its model has been read
    CALLCHK(hipEventRecord(res->ev[1], s));
    CALLCHK(hipStreamWaitEvent(sd, res->ev[1], 0));
    if (need_var_dyn) {                      // on h_dyn's own stream: the variance workspace belongs to the handle
        if (int rc = gpt_predict_all_dev(c.hd, a.x, M, nullptr, at[4], nullptr, nullptr, nullptr)) return rc;
        CALLCHK(hipEventRecord(res->ev[2], sd));
    }
    if (need_map) { if (int rc = gpt_predict_all_dev(c.hm, a.z, M, nullptr, u[PB_MAP_VAR], nullptr, need_jvar ? at[5] : nullptr, nullptr)) return rc; }
    if (need_var_dyn) CALLCHK(hipStreamWaitEvent(s, res->ev[2], 0));
    launch_pullback_variance(s, (int)D, a);
    CALLCHK(hipGetLastError());
    return GPT_OK;
}

}  // namespace

#define PULLBACK_CALL(c)                                                                                                            \
    PullbackCall c;                                                                                                                 \
    c.hm = h_map; c.hd = h_dyn; c.M = M; c.scale = scale; c.rtol = rtol; c.max_passes = max_passes; c.std_offset = std_offset;      \
    c.g = AffinePart{R, R_jac, c_src, c_dst};                                                                                       \
    {                                                                                                                               \
        const void* const all[PB_COUNT] = {y, x0, x, vel, f, det, residual, passes, status, var_dyn, map_var, vel_var_map, vel_var_dyn, \
                                           post_z, post_A, post_Jvar};                                                              \
        for (int k = 0; k < PB_COUNT; ++k) c.arr[k] = const_cast<void*>(all[k]);                                                    \
    }

extern "C" int gpt_pullback_policy_dev(gpt_handle* h_map, gpt_handle* h_dyn, const double* y, const double* x0, int64_t M, const double* R,
                                       const double* c_src, const double* c_dst, double scale, const double* R_jac, double rtol,
                                       int max_passes, double std_offset, double* x, double* vel, double* f, double* det, double* residual,
                                       int* passes, int* status, double* var_dyn, double* map_var, double* vel_var_map,
                                       double* vel_var_dyn, double* post_z, double* post_A, double* post_Jvar) {
    PULLBACK_CALL(c);
    if (int rc = pullback_check("gpt_pullback_policy_dev", c)) return rc;
    if (M == 0) return GPT_OK;
    return pullback_dev(c);
}

extern "C" int gpt_pullback_policy(gpt_handle* h_map, gpt_handle* h_dyn, const double* y, const double* x0, int64_t M, const double* R,
                                   const double* c_src, const double* c_dst, double scale, const double* R_jac, double rtol, int max_passes,
                                   double std_offset, double* x, double* vel, double* f, double* det, double* residual, int* passes,
                                   int* status, double* var_dyn, double* map_var, double* vel_var_map, double* vel_var_dyn, double* post_z,
                                   double* post_A, double* post_Jvar) {
    PULLBACK_CALL(c);
    if (int rc = pullback_check("gpt_pullback_policy", c)) return rc;
    if (M == 0) return GPT_OK;
    const size_t D = c.vm.p.D;
    if (!all_finite(y, (size_t)M * D) || (x0 && !all_finite(x0, (size_t)M * D)) || !affine_finite(c.g, D) || !std::isfinite(scale) ||
        !std::isfinite(rtol) || !std::isfinite(std_offset))
        return fail(GPT_E_ARG, "gpt_pullback_policy: y / x0 / the affine part / rtol / std_offset contain NaN or infinity");
    CallResources* const res = call_resources(h_map, CALL_PULLBACK, 3);
    if (!res) return GPT_E_HIP;
    ChunkStreams q;
    if (int rc = handle_copy_stream(h_map, !one_chunk(M), &q)) return rc;
    if (int rc = upload_affine(*res, 1, &c.g, 1, D, q.s)) return rc;
    // only what the caller asked for is staged and crosses the bus; the rest of what a later stage reads stays in the handle's scratch
    const size_t W = sizeof(double), I = sizeof(int);
    const size_t per[PB_COUNT] = {D * W, D * W, D * W, D * W, D * W, W, W, I, I, W, W, W, D * W, D * W, D * D * W, D * W};   // bytes per query, by PB_*
    StagedArray table[PB_COUNT];
    for (int k = 0; k < PB_COUNT; ++k) table[k] = StagedArray{c.arr[k], per[k], k < PB_INPUTS, 1};
    return run_chunked(res->st, q, table, M, [&](void* const* dev, int64_t m) {
        PullbackCall d = c;
        d.M = m; d.g = affine_slot(res->affine, 0);
        std::copy(dev, dev + PB_COUNT, d.arr);
        return pullback_dev(d);
    });
}
