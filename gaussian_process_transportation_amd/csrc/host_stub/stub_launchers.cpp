// Kernel launchers of the sanitizer builds (see host_stub/hip/hip_runtime.h): no arithmetic — each stand-in TOUCHES the
// memory its kernel would read and write, with the sizes the kernel derives from its arguments, so that AddressSanitizer
// checks the buffer sizing of the host orchestration (staging, model blob, slab / vslab / scratch of the variance plan).
#include "../gpt_common.h"
#include "../gpt_plan.h"
#include "../gpt_plan_i8.h"
#include "../gpt_fit_plan.h"
#include "../gpt_transport.h"
#include "../gpt_pullback.h"

namespace gpt {

static size_t esz(int dtype) { return dtype == DT_F32 ? sizeof(float) : sizeof(double); }
static void touch_w(void* p, size_t bytes) { if (p && bytes) memset(p, 0, bytes); }
static void touch_r(const void* p, size_t bytes) {
    if (!p || !bytes) return;
    volatile unsigned char acc = 0;
    const unsigned char* b = static_cast<const unsigned char*>(p);
    acc = acc + b[0]; acc = acc + b[bytes - 1]; acc = acc + b[bytes / 2];
}

size_t wf_elems(int NP) { const size_t nb = NP / WT; return nb * (nb + 1) / 2 * WT_TILE_DOUBLES; }
size_t wf_overrun_elems() { return WT_STEP_DOUBLES; }

void launch_gram(hipStream_t, const double* Xs, int D, int, int NP, int, double, double, double* K) {
    touch_r(Xs, (size_t)NP * xs_stride(D) * 8); touch_w(K, (size_t)NP * NP * 8);
}
void launch_scale_x(hipStream_t, const double* X, int N, int NP, int D, const double* inv_ls, double* Xs64, void* Xm, int dtype) {
    touch_r(X, (size_t)N * D * 8); touch_r(inv_ls, MAX_D * 8); touch_w(Xs64, (size_t)NP * xs_stride(D) * 8);
    touch_w(Xm, (size_t)NP * xs_stride(D) * esz(dtype));
}
void launch_dot(hipStream_t, const double* a, const double* b, int64_t n, double* out) { touch_r(a, (size_t)n * 8); touch_r(b, (size_t)n * 8); *out = 0.0; }
void launch_add_lower(hipStream_t, double* K, const double* S, int N, int NP) { touch_r(S, (size_t)N * N * 8); touch_w(K, (size_t)NP * NP * 8); }
void fit_aux_release(FitAux&) {}
size_t factor_scratch_doubles(int NP) { return factor_scratch_doubles_of(NP); }
// replays the plan's scratch regions (gpt_fit_plan.h) inside the buffer the orchestration allocated with factor_scratch_doubles
void launch_factor_inverse(hipStream_t, double* K, double* W, int NP, int* info, double* scratch, FitAux*, hipEvent_t) {
    touch_w(K, (size_t)NP * NP * 8); touch_w(W, (size_t)NP * NP * 8); *info = 0;
    const FitPlan pl = fit_plan(NP);
    for (const FitOp& op : pl.ops) {
        if (op.r0_size) touch_w(scratch + op.r0, op.r0_size * 8);
        if (op.r1_size) touch_w(scratch + op.r1, op.r1_size * 8);
    }
}
void launch_alpha(hipStream_t, const double* W, const double* Y4, int, int NP, double* tmp4, double* A4, double* scratch) {
    touch_r(W, (size_t)NP * NP * 8); touch_r(Y4, (size_t)NP * 32); touch_w(tmp4, (size_t)NP * 32); touch_w(A4, (size_t)NP * 32);
    touch_w(scratch, (size_t)(NP / 512) * NP * 32);
}
void launch_pack_w(hipStream_t, const double* W, int, int NP, void* Wf, int dtype, int task, double) {
    touch_r(W, (size_t)NP * NP * 8);
    touch_w(static_cast<unsigned char*>(Wf) + (size_t)task * wf_elems(NP) * esz(dtype), wf_elems(NP) * esz(dtype));
}
void launch_store4(hipStream_t, const double* src4, int rows, void* dst4, int dtype, int, int, int, double) {
    touch_r(src4, (size_t)rows * 32); touch_w(dst4, (size_t)rows * 4 * esz(dtype));
}
void launch_logdet(hipStream_t, const double* K, int, int NP, double* out) { touch_r(K, (size_t)NP * NP * 8); *out = 0.0; }
void launch_kinv(hipStream_t, const double* W, int NP, double* Kout) { touch_r(W, (size_t)NP * NP * 8); touch_w(Kout, (size_t)NP * NP * 8); }
void launch_cov(hipStream_t, const KernelParams& p, const double* Xs, const double* W, const double* Xq, int64_t M, int Mp, double* KsT,
                double* V, double* VtV, double* cov) {
    touch_r(Xs, (size_t)p.NP * xs_stride(p.D) * 8); touch_r(W, (size_t)p.NP * p.NP * 8); touch_r(Xq, (size_t)M * p.D * 8);
    touch_w(KsT, (size_t)p.NP * Mp * 8); touch_w(V, (size_t)p.NP * Mp * 8); touch_w(VtV, (size_t)Mp * Mp * 8); touch_w(cov, (size_t)M * M * 8);
}
void launch_lml_terms(hipStream_t, const double* Xs, int D, const double* A4, int npass, const double* Kinv, int, int NP, int, int, double,
                      double* partial, double* out) {
    touch_r(Xs, (size_t)NP * xs_stride(D) * 8); touch_r(A4, (size_t)npass * NP * 32); touch_r(Kinv, (size_t)NP * NP * 8);
    touch_w(partial, (size_t)(NP / 64) * (NP / 64) * LML_PARTIAL_STRIDE * 8); touch_w(out, LML_TERMS * 8);
}
void launch_mean_jac(hipStream_t, const KernelParams& p, const void* Xs, const void* A4, const void* Xq, int64_t M, void* mean, void* J) {
    const size_t e = esz(p.dtype);
    touch_r(Xs, (size_t)p.NP * xs_stride(p.D) * e); touch_r(A4, (size_t)((p.O + 3) / 4) * p.NP * 4 * e); touch_r(Xq, (size_t)M * p.D * e);
    touch_w(mean, (size_t)M * p.O * e); touch_w(J, (size_t)M * p.O * p.D * e);
}
void launch_inverse_newton(hipStream_t, const KernelParams& p, const double* Xs, const double* A4, const InverseArgs& a) {
    if (a.M <= 0) return;
    const size_t M = (size_t)a.M, D = (size_t)p.D;
    touch_r(Xs, (size_t)p.NP * 4 * 8); touch_r(A4, (size_t)p.NP * 4 * 8); touch_r(a.Y, M * D * 8); touch_r(a.Z0, M * D * 8);
    touch_w(a.Z, M * D * 8); touch_w(a.residual, M * 8); touch_w(a.det, M * 8); touch_w(a.passes, M * 4); touch_w(a.status, M * 4);
}
void launch_transport_affine(hipStream_t, int D_, const TransportArgs& a) {
    if (a.M <= 0) return;
    const size_t M = (size_t)a.M, D = (size_t)D_;
    touch_r(a.pos, M * D * 8); touch_r(a.R, D * D * 8); touch_r(a.c_src, D * 8); touch_r(a.c_dst, D * 8); touch_w(a.pos_rot, M * D * 8);
}
// k_push_forward: an array that is null is neither read nor written; J, Jvar and J_ori are read for the outputs that consume them
void launch_transport_push(hipStream_t, int D_, const TransportArgs& a) {
    if (a.M <= 0) return;
    const size_t M = (size_t)a.M, D = (size_t)D_;
    touch_r(a.R_jac, D * D * 8); touch_r(a.pos_rot, M * D * 8); touch_r(a.mean, M * D * 8); touch_w(a.pos_out, M * D * 8);
    if (a.det_vel || a.vel_out) touch_r(a.J, M * D * D * 8);
    if (a.vel_out || a.vel_var) touch_r(a.vel, M * D * 8);
    if (a.vel_var) touch_r(a.Jvar, M * D * 8);
    touch_w(a.vel_out, M * D * 8); touch_w(a.vel_var, M * 8); touch_w(a.det_vel, M * 8);
    if (a.ori_out || a.ori_gap || a.det_ori) touch_r(a.J_ori, M * D * D * 8);
    if (a.ori_out) touch_r(a.ori, M * 32);
    if (D == 3) { touch_w(a.ori_out, M * 32); touch_w(a.ori_gap, M * 8); }
    touch_w(a.det_ori, M * 8);
}
// k_pullback_velocity: both models' sources and alpha rows, the affine part, y and x0; an output that is null is not written
void launch_pullback_velocity(hipStream_t, const KernelParams& pm, const double* Xs_map, const double* A4_map, const KernelParams& pd,
                              const double* Xs_dyn, const double* A4_dyn, const PullbackArgs& a) {
    if (a.M <= 0) return;
    const size_t M = (size_t)a.M, D = (size_t)pm.D;
    touch_r(Xs_map, (size_t)pm.NP * 4 * 8); touch_r(A4_map, (size_t)pm.NP * 4 * 8);
    touch_r(Xs_dyn, (size_t)pd.NP * 4 * 8); touch_r(A4_dyn, (size_t)pd.NP * 4 * 8);
    touch_r(a.R, D * D * 8); touch_r(a.R_jac, D * D * 8); touch_r(a.c_src, D * 8); touch_r(a.c_dst, D * 8);
    touch_r(a.Y, M * D * 8); touch_r(a.X0, M * D * 8);
    touch_w(a.x, M * D * 8); touch_w(a.z, M * D * 8); touch_w(a.f, M * D * 8); touch_w(a.vel, M * D * 8); touch_w(a.A, M * D * D * 8);
    touch_w(a.det, M * 8); touch_w(a.residual, M * 8); touch_w(a.passes, M * 4); touch_w(a.status, M * 4);
}
// k_pullback_variance: f always; Jvar for vel_var_map; A and var_dyn for vel_var_dyn
void launch_pullback_variance(hipStream_t, int D_, const PullbackArgs& a) {
    if (a.M <= 0 || !(a.vel_var_map || a.vel_var_dyn)) return;
    const size_t M = (size_t)a.M, D = (size_t)D_;
    touch_r(a.R_jac, D * D * 8); touch_r(a.f, M * D * 8);
    if (a.vel_var_map) { touch_r(a.Jvar, M * D * 8); touch_w(a.vel_var_map, M * 8); }
    if (a.vel_var_dyn) { touch_r(a.A, M * D * D * 8); touch_r(a.var_dyn, M * 8); touch_w(a.vel_var_dyn, M * D * 8); }
}
void launch_var(hipStream_t, const KernelParams& p, const VarWorkspace& ws, const void* Xs, const void* Wf, const void* Xq, int64_t M,
                int ncomp, void* var, void* Jvar, void* dvar, const double* hdr) {
    if (M <= 0 || !ws.plan) return;
    const size_t e = esz(p.dtype);
    const VarPlanHost& pl = *ws.plan;
    touch_r(Xs, (size_t)p.NP * xs_stride(p.D) * e); touch_r(Xq, (size_t)M * p.D * e); touch_r(hdr, (16 + p.ntask) * 8);
    touch_r(Wf, ((size_t)p.ntask * wf_elems(p.NP) + wf_overrun_elems()) * e);
    const int* item_begin = pl.d.item_begin;
    touch_r(item_begin, (size_t)(pl.d.P + 1) * 4);
    for (int q = 0; q < pl.d.P; ++q) {
        touch_w(static_cast<unsigned char*>(ws.bscratch.p) + (size_t)q * p.NP * VAR_COLS * e, (size_t)p.NP * VAR_COLS * e);
        for (int i = item_begin[q]; i < item_begin[q + 1]; ++i) {
            const VarItem it = pl.d.items[i];
            if (it.vslot >= 0) touch_w(static_cast<unsigned char*>(ws.vslab.p) + (size_t)it.vslot * VAR_VSLOT * e, (size_t)VAR_VSLOT * e);
            if (it.slot >= 0) touch_w(static_cast<unsigned char*>(ws.slab.p) + (size_t)it.slot * VAR_SLOT * e, (size_t)VAR_SLOT * e);
        }
    }
    touch_w(ws.slab, (size_t)pl.d.nfull * p.ntask * VAR_SLOT * e);
    for (int i = 0; i < pl.d.n_splits; ++i) {
        const VarSplit sp = pl.d.splits[i];
        touch_r(static_cast<unsigned char*>(ws.vslab.p) + (size_t)sp.v_begin * VAR_VSLOT * e, (size_t)(sp.v_end - sp.v_begin) * VAR_VSLOT * e);
        touch_w(static_cast<unsigned char*>(ws.slab.p) + (size_t)sp.slot * VAR_SLOT * e, (size_t)VAR_SPLIT_SLOTS * VAR_SLOT * e);
    }
    for (int64_t c = 0; c < pl.d.ncb - pl.d.nfull; ++c)
        for (int t = 0; t < p.ntask; ++t) {
            const int b = pl.d.fin[2 * (c * p.ntask + t)], en = pl.d.fin[2 * (c * p.ntask + t) + 1];
            touch_r(static_cast<unsigned char*>(ws.slab.p) + (size_t)b * VAR_SLOT * e, (size_t)(en - b) * VAR_SLOT * e);
        }
    (void)var_cols_per_query(p.D, ncomp);
    touch_w(var, (size_t)M * p.ntask * e); touch_w(Jvar, (size_t)M * p.ntask * p.D * e); touch_w(dvar, (size_t)M * p.D * e);
}

void launch_var_i8_image(hipStream_t, const double* Wf, int NP, int, void* planes, double* rowscale, double* qscale, void* rowmax) {
    touch_r(Wf, wf_elems(NP) * 8);
    touch_w(planes, var_i8_plane_bytes(NP)); touch_w(rowscale, (size_t)NP * 8); touch_w(qscale, (size_t)NP * 8); touch_w(rowmax, (size_t)NP * 8);
}
void launch_var_i8(hipStream_t, const KernelParams& p, const VarI8PlanDev& plan, int, const void* planes, const double* rowscale,
                   const double* Xs, const double* Xq, int64_t M, double* slab, void* bimg, void* park, double* var, const double* hdr) {
    if (M <= 0) return;
    touch_r(planes, var_i8_plane_bytes(p.NP)); touch_r(rowscale, (size_t)p.NP * 8); touch_r(Xs, (size_t)p.NP * 4 * 8);
    touch_r(Xq, (size_t)M * p.D * 8); touch_r(hdr, 17 * 8);
    touch_w(slab, (size_t)plan.ncb * plan.nbi * I8_COLS * 8);
    touch_w(bimg, (size_t)var_i8_image_count(plan) * var_i8_bimg_bytes(p.NP)); touch_w(park, (size_t)plan.P * var_i8_park_bytes());
    touch_w(var, (size_t)M * 8);
}

}  // namespace gpt

#include "../../../include/gpt_hip.h"
// Stub only: allocations, streams and events created and not yet released (tests/asan_driver.py).
extern "C" long gpt_stub_live_objects(void) { return stub_live_objects; }

#ifdef GPT_STUB_ENTRY_POINTS
// The library of `make host-asan` holds the handle API alone (gpt_api.hip).  The one-shot units (gpt_svgp_train, gpt_svgp_surface,
// gpt_select, gpt_batch) and the GEMM's test hook (gpt_debug_dgemm, inside gpt_fit.hip) are not part of it; their entry points
// exist so that the ctypes loader, which binds every symbol of include/gpt_hip.h, loads this library too.  The host halves of
// the one-shot units run under the sanitizers in a program of their own: `make host-oneshot-asan`, the #else branch below.
extern "C" int gpt_svgp_train(int, const double*, const double*, int64_t, int, int, int, double*, double*, double*, double*, double*,
                              double*, const int64_t*, int64_t, const int64_t*, int64_t, double, double*) {
    gpt::set_last_error("gpt_svgp_train: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_svgp_elbo_grad(int, const double*, const double*, int64_t, int64_t, int, int, int, const double*, const double*,
                                  const double*, const double*, const double*, const double*, double*, double*, double*, double*,
                                  double*, double*, double*) {
    gpt::set_last_error("gpt_svgp_elbo_grad: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_svgp_surface_train(int, const double*, const double*, int64_t, int, int, int, double*, double*, double*, double*,
                                      double*, double*, const int64_t*, int64_t, const int64_t*, int64_t, double, double*) {
    gpt::set_last_error("gpt_svgp_surface_train: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_svgp_surface_elbo_grad(int, const double*, const double*, int64_t, int64_t, int, int, int, const double*,
                                          const double*, const double*, const double*, const double*, const double*, double*,
                                          double*, double*, double*, double*, double*, double*) {
    gpt::set_last_error("gpt_svgp_surface_elbo_grad: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_svgp_surface_predict(int, const double*, const double*, const double*, const double*, const double*, int, int, int,
                                        const double*, int64_t, double*, double*, double*) {
    gpt::set_last_error("gpt_svgp_surface_predict: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_select_greedy(int, const double*, int64_t, int, const double*, double, double, double, int, const int64_t*, int, int,
                                 int64_t*, double*, double*) {
    gpt::set_last_error("gpt_select_greedy: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_batch_lml_objective(int, const double*, const double*, const int64_t*, int64_t, int, int, const double*, int,
                                       const double*, const double*, double, int, double*, double*, int*) {
    gpt::set_last_error("gpt_batch_lml_objective: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_batch_fit(int, const double*, const double*, const int64_t*, int64_t, int, int, const double*, int, const double*,
                             const double*, double, int, double*, double*, double*, int*) {
    gpt::set_last_error("gpt_batch_fit: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_batch_predict(int, const double*, const double*, const int64_t*, int64_t, int, int, const double*, int,
                                 const double*, const double*, double, int, const double*, const int64_t*, double*, double*, double*,
                                 double*, double*, int*) {
    gpt::set_last_error("gpt_batch_predict: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_batch_optimize(int, const double*, const double*, const int64_t*, int64_t, int, int, int, const int*, const double*,
                                  int64_t, const double*, double, int, double, double, int, int, int, double*, double*, int*, int*, int*) {
    gpt::set_last_error("gpt_batch_optimize: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_batch_optimize_bounded(int, const double*, const double*, const int64_t*, int64_t, int, int, int, const int*, const double*,
                                          int64_t, const double*, double, int, double, double, int, int, int, double*, double*, int*, int*,
                                          int*) {
    gpt::set_last_error("gpt_batch_optimize_bounded: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_batch_fold_scan(int, const double*, const double*, const int64_t*, int64_t, int, const double*, int, const double*,
                                   const double*, double, int, const double*, const int64_t*, int64_t, int, double*, int64_t*, int64_t*,
                                   double*, double*, double*, double*, double*, int*, int*) {
    gpt::set_last_error("gpt_batch_fold_scan: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_pullback_chain_dev(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, int64_t, double, int, double,
                                      double*, double*, double*, int*, double*, double*, double*, double*, double*, double*, double*,
                                      double*, int*, int*, double*, double*) {
    gpt::set_last_error("gpt_pullback_chain_dev: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_pullback_chain(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, int64_t, double, int, double,
                                  double*, double*, double*, int*, double*, double*, double*, double*, double*, double*, double*, double*,
                                  int*, int*, double*, double*) {
    gpt::set_last_error("gpt_pullback_chain: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_policy_dev(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, int64_t, int64_t, double, double,
                                      int, double*, double*, double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_policy_dev: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_policy(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, int64_t, int64_t, double, double, int,
                                  double*, double*, double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_policy: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_stabilised_dev(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, int64_t, int64_t, double,
                                          double, int, double, double, double*, double*, double*, double*, double*, double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_stabilised_dev: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_stabilised(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, int64_t, int64_t, double, double,
                                      int, double, double, double*, double*, double*, double*, double*, double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_stabilised: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_sampled_dev(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, const double*, int64_t, int64_t,
                                       double, double, int, double, double*, double*, double*, double*, double*, double*, double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_sampled_dev: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_sampled(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, const double*, int64_t, int64_t, double,
                                   double, int, double, double*, double*, double*, double*, double*, double*, double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_sampled: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_pathwise_dev(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, const int*, int64_t, int64_t,
                                        double, double, int, int64_t, const double*, int64_t, const double*, const double*, double*, double*,
                                        double*, double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_pathwise_dev: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_rollout_pathwise(const gpt_chain_stage*, int, gpt_handle*, const double*, const double*, const int*, int64_t, int64_t, double,
                                    double, int, int64_t, const double*, int64_t, const double*, const double*, double*, double*, double*,
                                    double*, int*, int*) {
    gpt::set_last_error("gpt_rollout_pathwise: not in the host sanitizer build");
    return GPT_E_HIP;
}
extern "C" int gpt_debug_dgemm(int, int, int, int, int, int, double, const double*, int64_t, const double*, int64_t, double*, int64_t, int,
                               int*) {
    gpt::set_last_error("gpt_debug_dgemm: not in the host sanitizer build");
    return GPT_E_HIP;
}

#else
// The program of `make host-oneshot-asan` (oneshot_driver.cpp) links the real entry points of the one-shot units (gpt_*_host.hip);
// what follows stands in for their launchers (gpt_batch.h, gpt_batch_opt.h, gpt_select.h, gpt_svgp_train.h, gpt_svgp_surface.h).  As above, each
// walks the memory its kernels would read and write, deriving every offset and size from its arguments the way the kernels do,
// and writes the words the host reads back: status GPT_OK, failure flag and info untouched (no failure).  A layout the kernels
// rely on and no memory access shows (a task's workspace running into the next one's, a model in the wrong size class) ends
// the program through stub_check.
#include "../gpt_batch.h"
#include "../gpt_batch_opt.h"
#include "../gpt_fold_scan.h"
#include "../gpt_select.h"
#include "../gpt_svgp_train.h"
#include "../gpt_svgp_surface.h"
#include "../gpt_chain.h"
#include "../gpt_rollout.h"
#include "../gpt_rollout_stab.h"
#include "../gpt_rollout_sampled.h"
#include "../gpt_rollout_pathwise.h"
#include <cstdio>

namespace gpt {

// Test only (oneshot_driver.cpp): the batch member whose factor reports GPT_E_NOT_PD (-1: none), and whether the selection and
// the SVGP schedules stop on a non-positive pivot at their first step.
int stub_fail_model = -1;
bool stub_fail_flag = false;

#define stub_check(cond)                                                                          \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "stub_check failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); abort(); } \
    } while (0)

// ---- gpt_batch.hip ------------------------------------------------------------------------------------------------------------
void launch_bat_factor(hipStream_t, int, bool obj, int n_small, int n_large, const BatArgs& a) {
    for (int k = 0; k < n_small + n_large; ++k) {
        const int b = a.list[k];
        const int64_t n0 = a.n_begin[b], n = a.n_begin[b + 1] - n0;
        stub_check(n >= 1 && n <= (k < n_small ? BAT_SMALL_N : BAT_MAX_N));      // the LDS image of the size class
        touch_r(a.X + n0 * a.D, n * a.D * 8); touch_r(a.Y + n0 * a.O, n * a.O * 8);
        touch_r(a.ls + (int64_t)b * a.n_ls, a.n_ls * 8); touch_r(a.c + b, 8); touch_r(a.noise + b, 8);
        if (b == stub_fail_model) { a.status[b] = GPT_E_NOT_PD; continue; }       // bat_factor leaves before it writes anything else
        if (obj) touch_w(a.grad + (int64_t)b * (2 + a.n_ls), (2 + a.n_ls) * 8);
        else {
            touch_w(a.alpha + n0 * a.O, n * a.O * 8);
            if (a.L) touch_w(a.L + a.l_begin[b], n * n * 8);
            if (a.Wp) touch_w(a.Wp + a.w_begin[b], n * (n + 1) / 2 * 8);
        }
        if (a.lml) touch_w(a.lml + b, 8);
        a.status[b] = GPT_OK;
    }
}
void launch_bat_predict(hipStream_t, int, bool der, int tiles_small, int tiles_large, const BatPredArgs& a) {
    for (int t = 0; t < tiles_small + tiles_large; ++t) {
        const int b = a.tile_model[t];
        if (a.status[b] != GPT_OK) continue;
        const int64_t n0 = a.n_begin[b], n = a.n_begin[b + 1] - n0, qb = a.q_begin[b], Mb = a.q_begin[b + 1] - qb, q0 = a.tile_q0[t];
        stub_check(n >= 1 && n <= (t < tiles_small ? BAT_SMALL_N : BAT_MAX_N));
        stub_check(q0 >= 0 && q0 < Mb && q0 % BAT_QT == 0);
        const int64_t row = qb + q0, nq = (Mb - q0 < BAT_QT ? Mb - q0 : BAT_QT);
        touch_r(a.X + n0 * a.D, n * a.D * 8); touch_r(a.ls + (int64_t)b * a.n_ls, a.n_ls * 8); touch_r(a.c + b, 8); touch_r(a.noise + b, 8);
        touch_r(a.alpha + n0 * a.O, n * a.O * 8); touch_r(a.Wp + a.w_begin[b], n * (n + 1) / 2 * 8); touch_r(a.Xq + row * a.D, nq * a.D * 8);
        touch_w(a.mean ? a.mean + row * a.O : nullptr, nq * a.O * 8); touch_w(a.var ? a.var + row : nullptr, nq * 8);
        if (!der) continue;
        touch_w(a.J ? a.J + row * a.O * a.D : nullptr, nq * a.O * a.D * 8);
        touch_w(a.Jvar ? a.Jvar + row * a.D : nullptr, nq * a.D * 8); touch_w(a.dvar ? a.dvar + row * a.D : nullptr, nq * a.D * 8);
    }
}

// ---- gpt_batch_opt.hip --------------------------------------------------------------------------------------------------------
// Test only (oneshot_driver.cpp): run r ends in its (1 + r % stub_opt_launches)-th launch, so the relaunch loop of
// gpt_batch_optimize runs stub_opt_launches rounds and compacts its list of live runs between them.  A run whose model is
// stub_fail_model ends at once as GPT_OPT_NOT_PD_START.
int stub_opt_launches = 1;
int stub_opt_launch_count = 0;             // launches since the driver last reset it
void launch_bat_optimize(hipStream_t, int, int n_small, int n_large, const BatOptArgs& a) {
    const size_t P = 2 + (size_t)a.n_ls, rec = bat_opt_record((int)P);
    stub_opt_launch_count += (n_small > 0) + (n_large > 0);                      // one launch per size class present
    stub_check(n_small + n_large >= 1 && a.evals_per_launch >= 1 && a.max_ls == BAT_OPT_MAX_LS);
    stub_check(a.bounds_stride == 0 || a.bounds_stride == (int64_t)(2 * P));     // one box for all runs, or one per run
    for (int k = 0; k < n_small + n_large; ++k) {
        const int r = a.list[k], b = a.run_model[r];
        touch_r(a.bounds + (int64_t)r * a.bounds_stride, 2 * P * 8);
        const int64_t n0 = a.n_begin[b], n = a.n_begin[b + 1] - n0;
        stub_check(n >= 1 && n <= (k < n_small ? BAT_SMALL_N : BAT_MAX_N));      // the LDS image of the size class
        stub_check(k == 0 || a.list[k - 1] < r || k == n_small);                  // a run once per launch: each class in rising order
        stub_check(a.status[r] == BAT_OPT_LIVE);                                  // a run that has ended is not launched again
        touch_r(a.X + n0 * a.D, n * a.D * 8); touch_r(a.Y + n0 * a.O, n * a.O * 8);
        int* cn = a.cnt + (size_t)r * BAT_OPT_CNT;
        if (cn[1] == 0) { stub_check(cn[0] == 0 && cn[2] == 0 && a.iters[r] == 0 && a.evals[r] == 0); touch_r(a.theta + r * P, P * 8); }
        touch_w(a.rec + r * rec, rec * 8);
        ++cn[1];
        const bool not_pd = b == stub_fail_model;
        if (!not_pd && cn[1] < 1 + r % stub_opt_launches) continue;
        if (!not_pd) touch_w(a.theta + r * P, P * 8);                             // a start that is not PD stays in theta
        touch_w(a.lml + r, 8); touch_w(a.iters + r, 4);
        a.evals[r] = cn[1];
        a.status[r] = not_pd ? GPT_OPT_NOT_PD_START : GPT_OPT_PGTOL;
    }
}

// ---- gpt_fold_scan.hip --------------------------------------------------------------------------------------------------------
// Test only (oneshot_driver.cpp): the batch member whose surrogate matrix alone reports GPT_E_NOT_PD (-1: none).
int stub_fail_surrogate = -1;
void launch_fs_factor(hipStream_t, int n_small, int n_large, const FoldScanArgs& a) {
    stub_check(a.D >= 1 && a.D <= FS_MAX_D && (a.surrogate == 0) == (a.Xs == nullptr) && (a.surrogate == 0) == (a.sur_status == nullptr));
    for (int k = 0; k < n_small + n_large; ++k) {
        const int b = a.list[k];
        const int64_t n0 = a.n_begin[b], n = a.n_begin[b + 1] - n0;
        stub_check(n >= 1 && n <= (k < n_small ? BAT_SMALL_N : BAT_MAX_N));      // the LDS image of the size class
        touch_r(a.X + n0 * a.D, n * a.D * 8); touch_r(a.Y + n0 * a.D, n * a.D * 8);
        touch_r(a.ls + (int64_t)b * a.n_ls, a.n_ls * 8); touch_r(a.c + b, 8); touch_r(a.noise + b, 8);
        if (b == stub_fail_model) { a.status[b] = GPT_E_NOT_PD; continue; }       // fs_factor leaves before the surrogate's pass
        touch_w(a.alpha + n0 * a.D, n * a.D * 8);
        a.status[b] = GPT_OK;
        if (!a.surrogate) continue;
        touch_r(a.Xs + n0 * a.D, n * a.D * 8); touch_r(a.Ys + n0 * a.D, n * a.D * 8);
        if (b == stub_fail_surrogate) { a.sur_status[b] = GPT_E_NOT_PD; continue; }
        touch_w(a.beta + n0 * a.D, n * a.D * 8);
        a.sur_status[b] = GPT_OK;
    }
}
void launch_fs_scan(hipStream_t, int tiles_small, int tiles_large, int64_t B, const FoldScanArgs& a) {
    for (int t = 0; t < tiles_small + tiles_large; ++t) {
        const int b = a.tile_model[t];
        if (a.status[b] != GPT_OK) continue;
        const int64_t n0 = a.n_begin[b], n = a.n_begin[b + 1] - n0, ob = a.o_begin[b], Mb = a.o_begin[b + 1] - ob, q0 = a.tile_q0[t];
        stub_check(n >= 1 && n <= (t < tiles_small ? BAT_SMALL_N : BAT_MAX_N));
        stub_check(q0 >= 0 && q0 < Mb && q0 % BAT_QT == 0 && t == a.tile_first[b] + q0 / BAT_QT);
        const bool sur = a.surrogate && a.sur_status[b] == GPT_OK;
        const int64_t nq = (Mb - q0 < BAT_QT ? Mb - q0 : BAT_QT), row = ob + q0;
        touch_r(a.X + n0 * a.D, n * a.D * 8); touch_r(a.alpha + n0 * a.D, n * a.D * 8);
        if (sur) { touch_r(a.Xs + n0 * a.D, n * a.D * 8); touch_r(a.beta + n0 * a.D, n * a.D * 8); }
        touch_r(a.ls + (int64_t)b * a.n_ls, a.n_ls * 8); touch_r(a.c + b, 8);
        touch_r(a.Xq + ((a.shared ? 0 : ob) + q0) * a.D, nq * a.D * 8);
        touch_w(a.det ? a.det + row : nullptr, nq * 8); touch_w(a.z ? a.z + row * a.D : nullptr, nq * a.D * 8);
        if (sur) touch_w(a.err ? a.err + row : nullptr, nq * 8);
        touch_w(a.part + (int64_t)t * FS_PART_D, FS_PART_D * 8); touch_w(a.ipart + (int64_t)t * FS_PART_I, FS_PART_I * 4);
    }
    for (int64_t b = 0; b < B; ++b) {
        if (a.status[b] != GPT_OK) continue;
        const int64_t Mb = a.o_begin[b + 1] - a.o_begin[b], nt = (Mb + BAT_QT - 1) / BAT_QT;
        stub_check(nt == 0 || a.tile_model[a.tile_first[b]] == b);
        touch_r(a.part + (int64_t)a.tile_first[b] * FS_PART_D, nt * FS_PART_D * 8); touch_r(a.ipart + (int64_t)a.tile_first[b] * FS_PART_I, nt * FS_PART_I * 4);
        touch_w(a.min_det + b, 8); touch_w(a.argmin + b, 8); touch_w(a.n_fold + b, 8);
        if (a.surrogate && a.sur_status[b] == GPT_OK) { touch_w(a.err_sum + b, 8); touch_w(a.err_max + b, 8); }
    }
}

// ---- gpt_select.hip -----------------------------------------------------------------------------------------------------------
void launch_sel_schedule(hipStream_t, const SelArgs& a, const double* X, const double* inv_ls, double* Xs, int D, int n_total) {
    const size_t N = a.N, mp = a.mp, stride = a.stride;
    stub_check(a.Xs == Xs && mp % 2 == 0 && (int)mp >= n_total && stride % 2 == 0 && (int)stride >= D);   // sel_column's 16-byte loads
    touch_r(X, N * D * 8); touch_r(inv_ls, D * 8); touch_w(Xs, N * stride * 8);
    touch_w(a.d, N * 8); memset(a.alive, 1, N); a.pivd[0] = a.base_var;
    for (int j = 0; j < n_total; ++j) {
        if (*a.fail) return;
        if (stub_fail_flag) { *a.fail = j + 1; return; }
        const int p = a.selected[j], lpr = j <= 32 ? 8 : (j <= 128 ? 16 : 64), groups = SEL_NT / lpr;
        stub_check(p >= 0 && (size_t)p < N);
        const size_t want = (N + groups - 1) / groups, G = want < (size_t)SEL_MAX_WG ? want : (size_t)SEL_MAX_WG;
        touch_r(a.pivd + j, 8); touch_r(a.Xs + p * stride, stride * 8);
        for (size_t i = 0; i < N; ++i) {                      // a row's first j entries in pairs, then column j
            touch_r(a.P + i * mp, (size_t)((j + 1) & ~1) * 8); touch_r(a.Xs + i * stride, stride * 8);
            touch_w(a.P + i * mp + j, 8); touch_w(a.d + i, 8);
        }
        a.alive[p] = 0;
        touch_w(a.part_d, G * 8); touch_w(a.part_i, G * 4);
        if (j + 1 == n_total) break;
        if (j + 1 >= a.n_pre) {                               // sel_next: the lowest row still alive stands in for the maximum
            size_t i = 0;
            while (i < N && !a.alive[i]) ++i;
            stub_check(i < N);
            a.selected[j + 1] = (int)i;
        }
        a.pivd[j + 1] = a.d[a.selected[j + 1]];
    }
}

// ---- gpt_chain.hip ------------------------------------------------------------------------------------------------------------
// k_chain_velocity: every stage's and the dynamics' sources and alpha rows, every affine part, y and x0; an output that is null is
// not written; a per-stage array holds K * M rows
void launch_chain_velocity(hipStream_t, int D_, const ChainArgs& a) {
    if (a.M <= 0) return;
    stub_check(a.K >= 1 && a.K <= CHAIN_MAX && a.vel && a.status);
    const size_t M = (size_t)a.M, D = (size_t)D_, K = (size_t)a.K;
    auto model = [](const ChainModel& m) {
        const size_t NP = ((size_t)m.N + PAD_N - 1) / PAD_N * PAD_N;
        touch_r(m.Xs, NP * 4 * 8); touch_r(m.A4, NP * 4 * 8);
    };
    for (size_t k = 0; k < K; ++k) {
        const ChainStage& S = a.st[k];
        model(S.m);
        touch_r(S.R, D * D * 8); touch_r(S.R_jac, D * D * 8); touch_r(S.c_src, D * 8); touch_r(S.c_dst, D * 8);
    }
    model(a.dyn);
    touch_r(a.Y, M * D * 8); touch_r(a.X0, M * D * 8);
    touch_w(a.x, M * D * 8); touch_w(a.f, M * D * 8); touch_w(a.vel, M * D * 8); touch_w(a.status, M * 4);
    touch_w(a.stage_x, K * M * D * 8); touch_w(a.stage_z, K * M * D * 8); touch_w(a.stage_A, K * M * D * D * 8);
    touch_w(a.stage_status, K * M * 4); touch_w(a.stage_passes, K * M * 4); touch_w(a.stage_residual, K * M * 8); touch_w(a.stage_det, K * M * 8);
}
// k_chain_variance: f, Jvar_k and (K > 1) A_k for vel_var_map; A_k and var_dyn for vel_var_dyn
void launch_chain_variance(hipStream_t, int D_, const ChainArgs& a) {
    if (a.M <= 0 || !(a.vel_var_map || a.vel_var_dyn)) return;
    const size_t M = (size_t)a.M, D = (size_t)D_, K = (size_t)a.K;
    for (size_t k = 0; k < K; ++k) touch_r(a.st[k].R_jac, D * D * 8);
    if (a.vel_var_map) {
        stub_check(a.f && a.stage_Jvar && (K == 1 || a.stage_A));
        touch_r(a.f, M * D * 8); touch_r(a.stage_Jvar, K * M * D * 8); touch_w(a.vel_var_map, M * D * 8);
    }
    if (a.vel_var_map && K > 1) touch_r(a.stage_A, K * M * D * D * 8);
    if (a.vel_var_dyn) {
        stub_check(a.stage_A && a.var_dyn);
        touch_r(a.stage_A, K * M * D * D * 8); touch_r(a.var_dyn, M * 8); touch_w(a.vel_var_dyn, M * D * 8);
    }
}

// ---- gpt_rollout.hip ----------------------------------------------------------------------------------------------------------
// k_rollout: the models and affine parts as k_chain_velocity; a launch with t_begin == 0 reads y0 and x0 and writes row 0 of every
// path, a later one reads steps_done and, of the trajectories alive, `state` and path row t_begin.  The stand-in ends no
// trajectory: every launch writes its steps' rows, steps_done = t_end and status, and `state` when another launch follows
int stub_rollout_launch_count = 0;         // launches since the driver last reset it
void launch_rollout(hipStream_t, int D_, const RolloutArgs& a) {
    if (a.M <= 0) return;
    ++stub_rollout_launch_count;
    stub_check(a.K >= 0 && a.K <= CHAIN_MAX && a.path && a.steps_done && a.status);
    stub_check(a.T >= 0 && a.t_begin >= 0 && a.t_begin <= a.t_end && a.t_end <= a.T && (a.t_begin < a.t_end || a.T == 0));
    stub_check(a.M * ((int64_t)a.T + 1) < ((int64_t)1 << 31));
    const size_t M = (size_t)a.M, D = (size_t)D_, T = (size_t)a.T, t0 = (size_t)a.t_begin, t1 = (size_t)a.t_end;
    auto model = [](const ChainModel& m) {
        const size_t NP = ((size_t)m.N + PAD_N - 1) / PAD_N * PAD_N;
        touch_r(m.Xs, NP * 4 * 8); touch_r(m.A4, NP * 4 * 8);
    };
    for (int k = 0; k < a.K; ++k) {
        const ChainStage& S = a.st[k];
        model(S.m);
        touch_r(S.R, D * D * 8); touch_r(S.R_jac, D * D * 8); touch_r(S.c_src, D * 8); touch_r(S.c_dst, D * 8);
    }
    model(a.dyn);
    if (t0 == 0) { touch_r(a.Y0, M * D * 8); touch_r(a.X0, M * D * 8); }
    else { stub_check(a.state); touch_r(a.state, M * D * 8); }
    for (size_t m = 0; m < M; ++m) {
        if (t0 == 0) touch_w(a.path + m * (T + 1) * D, D * 8);
        else { stub_check(a.steps_done[m] == a.t_begin); touch_r(a.path + (m * (T + 1) + t0) * D, D * 8); }
        touch_w(a.path + (m * (T + 1) + t0 + 1) * D, (t1 - t0) * D * 8);
        if (a.vel) touch_w(a.vel + (m * T + t0) * D, (t1 - t0) * D * 8);
        if (a.x) touch_w(a.x + (m * T + t0) * D, (t1 - t0) * D * 8);
        a.steps_done[m] = a.t_end;
        a.status[m] = 0;
    }
    if (t1 < T) { stub_check(a.state); touch_w(a.state, M * D * 8); }
}

// ---- gpt_rollout_stab.hip -----------------------------------------------------------------------------------------------------
// k_rollout_stab: what k_rollout reads and writes, and of the dynamics also the packed inverse factor (every tile of its NP, which
// the kernel's image in LDS bounds); f, var (one double per step) and dvar are written where they are asked for
void launch_rollout_stab(hipStream_t s, int D_, const RolloutStabArgs& sa) {
    const RolloutArgs& a = sa.r;
    if (a.M <= 0) return;
    stub_check(sa.Wf && sa.NP % PAD_N == 0 && sa.NP >= a.dyn.N && sa.NP <= ROLLOUT_STAB_MAX_N && a.dyn.N >= 1);
    stub_check(sa.gain >= 0.0 && sa.gain <= 1e300 && sa.std_offset == sa.std_offset);
    const size_t nb = (size_t)sa.NP / WT;
    touch_r(sa.Wf, nb * (nb + 1) / 2 * WT_TILE_DOUBLES * 8);
    const size_t M = (size_t)a.M, D = (size_t)D_, T = (size_t)a.T, t0 = (size_t)a.t_begin, t1 = (size_t)a.t_end;
    for (size_t m = 0; m < M; ++m) {
        if (sa.f) touch_w(sa.f + (m * T + t0) * D, (t1 - t0) * D * 8);
        if (sa.var) touch_w(sa.var + m * T + t0, (t1 - t0) * 8);
        if (sa.dvar) touch_w(sa.dvar + (m * T + t0) * D, (t1 - t0) * D * 8);
    }
    launch_rollout(s, D_, a);                         // the mean rollout's arrays, its checks and its launch count
}

// ---- gpt_rollout_sampled.hip --------------------------------------------------------------------------------------------------
// k_rollout_sampled: what k_rollout reads and writes (x always: the caller's array or scratch), of the dynamics also the packed
// inverse factor, the normals of the launch's steps, and the scratch of the call: u of the steps so far of every workgroup, the
// transposed factor up to the launch's last row, the cross products; f, pvar, cvar and chol are written where they are asked for
void launch_rollout_sampled(hipStream_t s, int D_, const RolloutSampledArgs& sa) {
    const RolloutArgs& a = sa.r;
    if (a.M <= 0) return;
    stub_check(sa.Wf && sa.NP % PAD_N == 0 && sa.NP >= a.dyn.N && sa.NP <= ROLLOUT_STAB_MAX_N && a.dyn.N >= 1);
    stub_check(sa.nugget >= 0.0 && sa.nugget <= 1e300 && a.T <= ROLLOUT_SAMPLED_MAX_T);
    const size_t nb = (size_t)sa.NP / WT;
    touch_r(sa.Wf, nb * (nb + 1) / 2 * WT_TILE_DOUBLES * 8);
    const size_t M = (size_t)a.M, D = (size_t)D_, T = (size_t)a.T, t0 = (size_t)a.t_begin, t1 = (size_t)a.t_end;
    const size_t wgs = (M + ROLLOUT_SAMPLED_TILE - 1) / ROLLOUT_SAMPLED_TILE, ustep = (size_t)sampled_u_rows(a.dyn.N) * 16;
    if (T > 0) {
        stub_check(a.x && sa.normals && sa.U && sa.Gt && sa.cb);
        for (size_t g = 0; g < wgs; ++g) {
            touch_r(sa.U + g * T * ustep, t0 * ustep * 8);
            touch_w(sa.U + (g * T + t0) * ustep, (t1 - t0) * ustep * 8);
            touch_w(sa.cb + g * (T + 1) * 16, (t1 + 1) * 16 * 8);
        }
    }
    for (size_t m = 0; m < M; ++m) {
        touch_r(sa.normals + m * T * D, t1 * D * 8);
        if (t0 > 0) touch_r(a.x + m * T * D, t0 * D * 8);
        for (size_t t = t0; t < t1; ++t)
            for (size_t r = 0; r <= t; ++r) touch_w(sa.Gt + (m * T + r) * sampled_ld(a.T) + t, 8);
        if (sa.f) touch_w(sa.f + (m * T + t0) * D, (t1 - t0) * D * 8);
        if (sa.pvar) touch_w(sa.pvar + m * T + t0, (t1 - t0) * 8);
        if (sa.cvar) touch_w(sa.cvar + m * T + t0, (t1 - t0) * 8);
        if (sa.chol) touch_w(sa.chol + (m * T + t0) * T, (t1 - t0) * T * 8);
    }
    launch_rollout(s, D_, a);                         // the mean rollout's arrays, its checks and its launch count
}

// ---- gpt_rollout_pathwise.hip -------------------------------------------------------------------------------------------------
// k_rollout_pathwise: what k_rollout reads and writes, with the dynamics' alpha rows replaced by the image of each path's function
// (whole images of NP rows), func of every path, the frequencies and the amplitudes of the functions in use; f is written where
// it is asked for
void launch_rollout_pathwise(hipStream_t s, int D_, const RolloutPathwiseArgs& pa) {
    const RolloutArgs& a = pa.r;
    if (a.M <= 0) return;
    const size_t NP = ((size_t)a.dyn.N + PAD_N - 1) / PAD_N * PAD_N;
    stub_check(pa.S >= 1 && pa.J >= 0 && pa.J <= PATHWISE_MAX_FREQ && pa.func && pa.V4 && pa.image == NP * 4);
    stub_check(pa.J == 0 || (pa.omega && pa.amp));
    const size_t M = (size_t)a.M, D = (size_t)D_, T = (size_t)a.T, t0 = (size_t)a.t_begin, t1 = (size_t)a.t_end, J = (size_t)pa.J;
    touch_r(pa.func, M * 4);
    touch_r(pa.omega, J * D * 8);
    for (size_t m = 0; m < M; ++m) {
        stub_check(pa.func[m] >= 0 && pa.func[m] < pa.S);
        const size_t fn = (size_t)pa.func[m];
        touch_r(pa.V4 + fn * pa.image, pa.image * 8);
        touch_r(pa.amp + fn * J * 2 * D, J * 2 * D * 8);
        if (pa.f) touch_w(pa.f + (m * T + t0) * D, (t1 - t0) * D * 8);
    }
    launch_rollout(s, D_, a);                         // the mean rollout's arrays, its checks and its launch count
}

// ---- gpt_svgp_train.hip, gpt_svgp_surface.hip ---------------------------------------------------------------------------------
// the rows of one step's batch: X and Y through the schedule
static void touch_batch(const double* X, const double* Y, const int* idx, int N, int D, int T, int b0, int b) {
    for (int k = 0; k < b; ++k) {
        const int row = idx[b0 + k];
        stub_check(row >= 0 && row < N);
        touch_r(X + (size_t)row * D, D * 8); touch_r(Y + (size_t)row * T, T * 8);
    }
}
void launch_svgp_steps(hipStream_t, const SvArgs& a, const int64_t* bb, int64_t n_steps, int apply, double) {
    const int64_t D = a.D, T = a.T, Zn = a.Zn, ZZ = Zn * Zn, ZB = Zn * a.bmax;
    stub_check(a.n_shared == D + Zn * D + 1 && a.task_stride == 2 + Zn + ZZ && a.part_stride == 2 + D + Zn * D);
    stub_check(Zn <= SV_MAX_Z && a.bmax <= SV_MAX_B);
    for (int64_t st = 0; st < n_steps; ++st) {
        if (*a.fail != INT_MAX) return;
        if (stub_fail_flag) { *a.fail = (int)st * 64; return; }
        const int b0 = (int)(bb[st] - bb[0]), b = (int)(bb[st + 1] - bb[st]);
        stub_check(b >= 1 && b <= a.bmax);
        touch_batch(a.X, a.Y, a.idx, a.N, a.D, a.T, b0, b);
        // svgp_shared_step: the shared head of theta and its gradient; svgp_task_step: task t's own slice of each
        touch_r(a.theta, a.n_shared * 8); touch_w(a.grad, a.n_shared * 8);
        if (apply) for (double* v : {a.theta, a.m1, a.m2}) touch_w(v, a.n_shared * 8);
        for (int64_t t = 0; t < T; ++t) {
            const int64_t th0 = a.n_shared + t * a.task_stride, th_n = 2 + Zn + ZZ;   // raw_os, raw_noise_t, m, C
            touch_r(a.theta + th0, th_n * 8); touch_w(a.grad + th0, th_n * 8);
            if (apply) for (double* v : {a.theta, a.m1, a.m2}) touch_w(v + th0, th_n * 8);
            double* w = a.ws + t * a.ws_stride;                      // M0, M1, M2 | Kx, A, U, Ab, B | Xb | yb, as svgp_task_step carves them
            for (int q = 0; q < 3; ++q, w += ZZ) touch_w(w, ZZ * 8);
            for (int q = 0; q < 5; ++q, w += ZB) touch_w(w, Zn * b * 8);
            touch_w(w, b * D * 8); w += a.bmax * D;
            touch_w(w, b * 8); w += a.bmax;
            stub_check(w - (a.ws + t * a.ws_stride) <= a.ws_stride);
            touch_w(a.part + t * a.part_stride, (2 + D + Zn * D) * 8);
        }
        touch_w(a.loss + st, 8);
    }
}

void launch_sf_train(hipStream_t s, const SfArgs& a, const int64_t* bb, int64_t n_steps, int apply, double) {
    const int64_t D = a.D, T = a.T, Zn = a.Zn, NP = a.NP, BP = a.BP, NN = NP * NP, NB_ = NP * BP, nz = Zn * D;
    stub_check(NP % PAD_N == 0 && NP >= Zn && BP % 64 == 0 && 2 + D <= SF_HDR);
    stub_check(a.SH >= nz + 1 && a.SH % 2 == 0 && a.task_stride == SF_HDR + NP + NN && a.part_stride == 2 + nz);
    for (int64_t st = 0; st < n_steps; ++st) {
        if (*a.fail != INT_MAX) return;
        const int b0 = (int)(bb[st] - bb[0]), b = (int)(bb[st + 1] - bb[st]);
        stub_check(b >= 1 && b <= BP);
        touch_batch(a.X, a.Y, a.idx, a.N, a.D, a.T, b0, b);
        touch_r(a.theta, a.SH * 8); touch_w(a.grad, a.SH * 8);                    // the shared head: Z, raw_noise_global, pad to SH
        if (apply) for (double* v : {a.theta, a.m1, a.m2}) touch_w(v, a.SH * 8);
        for (int64_t t = 0; t < T; ++t) {
            const int64_t th0 = a.SH + t * a.task_stride;                         // task t: header (SF_HDR), m (NP), C (NP x NP)
            touch_r(a.theta + th0, (SF_HDR + NP) * 8); touch_w(a.grad + th0, (SF_HDR + NP) * 8);
            if (apply) for (double* v : {a.theta, a.m1, a.m2}) touch_w(v + th0, a.task_stride * 8);
            launch_factor_inverse(s, a.K, a.W, (int)NP, a.info + t, a.scr, nullptr, nullptr);
            if (stub_fail_flag) { a.info[t] = 1; *a.fail = (int)(st * 64 + t); return; }
            for (double* p : {a.Q, a.M2, a.theta + a.SH + t * a.task_stride + SF_HDR + NP, a.grad + a.SH + t * a.task_stride + SF_HDR + NP})
                touch_w(p, NN * 8);
            for (double* p : {a.Kx, a.A, a.U, a.CU, a.Ab, a.B}) touch_w(p, NB_ * 8);
            touch_w(a.stat, 3 * b * 8); touch_w(a.rbuf, BP * 8);
            touch_w(a.klrow, Zn * 8); touch_w(a.rowpart, Zn * (1 + D) * 8);          // one entry per inducing row (the host sizes both with NP)
            touch_w(a.sc, 4 * 8); touch_w(a.part + t * a.part_stride, (2 + nz) * 8);
        }
        touch_w(a.loss + st, 8);
    }
}
void launch_sf_pred_factor(hipStream_t s, const SfPredArgs& p) {
    launch_factor_inverse(s, p.K, p.W, p.NP, p.info, p.scr, nullptr, nullptr);
    if (stub_fail_flag) *p.info = 1;
}
void launch_sf_pred_chunks(hipStream_t, const SfPredArgs& p, int t, double) {
    const size_t NP = p.NP, MC = p.MC, D = p.D, T = p.T;
    stub_check(MC % 64 == 0 && MC <= (size_t)SF_PRED_CHUNK && t >= 0 && t < p.T);
    touch_r(p.W, NP * NP * 8); touch_r(p.C, NP * NP * 8); touch_r(p.m, NP * 8); touch_r(p.il, D * 8); touch_r(p.Z, p.Zn * D * 8);
    touch_w(p.beta, NP * 8);
    for (int64_t q0 = 0; q0 < p.M; q0 += MC) {
        const size_t nq = (size_t)(p.M - q0 < (int64_t)MC ? p.M - q0 : MC);
        touch_r(p.Xq + q0 * D, nq * D * 8);
        for (double* panel : {p.Kq, p.Aq, p.Vq}) touch_w(panel, NP * MC * 8);
        for (size_t q = q0; q < q0 + nq; ++q) {                // column t of the (M, T) outputs
            touch_w(p.mean + q * T + t, 8);
            if (p.var) touch_w(p.var + q * T + t, 8);
            if (p.J) touch_w(p.J + (q * T + t) * D, D * 8);
        }
    }
}

}  // namespace gpt
#endif
