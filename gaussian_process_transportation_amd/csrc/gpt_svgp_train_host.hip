// gpt_svgp_train and gpt_svgp_elbo_grad (include/gpt_hip.h): argument checks, the flat theta layout packed on the way in and
// scattered on the way out, the per-task workspace and partials, the read-back.  Host code only (the kernels: gpt_svgp_train.hip,
// reached through the launcher of gpt_svgp_train.h), so it also compiles under g++ against host_stub/ and runs under the
// sanitizers (make host-oneshot-asan).
#include "gpt_svgp_train.h"

using namespace gpt;

namespace {

// The whole schedule: shared by gpt_svgp_train (apply = 1) and gpt_svgp_elbo_grad (one step, apply = 0).
int run(int device, const char* who, const SvgpCall& c) {
    const std::string w = who;
    int bmax = 0;
    if (int rc = svgp_validate(w, c, SV_LIMITS, c.D, &bmax)) return rc;
    if (int rc = use_device(w, device)) return rc;
    const int D = c.D, T = c.T, Zn = c.Zn;

    const int64_t ZZ = (int64_t)Zn * Zn;
    const int64_t n_shared = D + (int64_t)Zn * D + 1, task_stride = 2 + Zn + ZZ, n_theta = n_shared + T * task_stride;
    std::vector<double> th(n_theta);
    for (int d = 0; d < D; ++d) th[d] = c.raw_ls[d];
    for (int64_t e = 0; e < (int64_t)Zn * D; ++e) th[D + e] = c.Z[e];
    th[n_shared - 1] = c.raw_noise[T];
    for (int t = 0; t < T; ++t) {
        double* p = th.data() + n_shared + t * task_stride;
        p[0] = c.raw_os[t];
        p[1] = c.raw_noise[t];
        for (int i = 0; i < Zn; ++i) p[2 + i] = c.m[(int64_t)t * Zn + i];
        for (int64_t e = 0; e < ZZ; ++e) {
            const int i = (int)(e / Zn), j = (int)(e % Zn);
            p[2 + Zn + e] = j > i ? 0.0 : c.C[t * ZZ + e];          // the strict upper triangle is not a parameter
        }
    }
    std::vector<int> idx32;
    CallBuffers buf;
    CALLCHK(buf.open());
    const hipStream_t s = buf.stream;
    SvgpDevice dev;
    if (int rc = svgp_upload(buf, c, th, &idx32, &dev)) return rc;
    SvArgs a{};
    a.X = dev.X; a.Y = dev.Y; a.idx = dev.idx; a.loss = dev.loss; a.fail = dev.fail;
    a.theta = dev.theta; a.grad = dev.grad; a.m1 = dev.m1; a.m2 = dev.m2;
    a.N = (int)c.N; a.D = D; a.T = T; a.Zn = Zn; a.bmax = bmax; a.num_data = (double)c.num_data;
    a.n_shared = n_shared; a.task_stride = task_stride; a.part_stride = 2 + D + (int64_t)Zn * D;
    a.ws_stride = 3 * ZZ + 5 * (int64_t)Zn * bmax + (int64_t)bmax * D + bmax;
    CALLCHK(buf.alloc(&a.part, (size_t)T * a.part_stride));
    CALLCHK(buf.alloc(&a.ws, (size_t)T * a.ws_stride));

    launch_svgp_steps(s, a, c.bb, c.n_steps, c.apply, c.lr);
    std::vector<double> out(n_theta);
    double* dst[6];
    if (int rc = svgp_read_back(w, s, c, dev, &out, dst)) return rc;
    // scatter the flat vector (parameters, or gradients) back into the caller's arrays
    if (dst[3]) for (int d = 0; d < D; ++d) dst[3][d] = out[d];
    if (dst[0]) for (int64_t e = 0; e < (int64_t)Zn * D; ++e) dst[0][e] = out[D + e];
    if (dst[5]) dst[5][T] = out[n_shared - 1];
    for (int t = 0; t < T; ++t) {
        const double* p = out.data() + n_shared + t * task_stride;
        if (dst[4]) dst[4][t] = p[0];
        if (dst[5]) dst[5][t] = p[1];
        if (dst[1]) for (int i = 0; i < Zn; ++i) dst[1][(int64_t)t * Zn + i] = p[2 + i];
        if (dst[2])
            for (int64_t e = 0; e < ZZ; ++e) {
                const int i = (int)(e / Zn), j = (int)(e % Zn);
                if (j <= i || !c.apply) dst[2][t * ZZ + e] = p[2 + Zn + e];      // parameters: the upper triangle stays as passed
            }
    }
    return GPT_OK;
}

}  // namespace

extern "C" int gpt_svgp_train(int device, const double* X, const double* Y, int64_t N, int D, int T, int n_inducing, double* Z, double* m,
                              double* C, double* raw_lengthscale, double* raw_outputscale, double* raw_noise, const int64_t* idx, int64_t n_idx,
                              const int64_t* batch_begin, int64_t n_steps, double lr, double* loss_trace) {
    SvgpCall c{};
    c.X = X; c.Y = Y; c.N = N; c.num_data = N; c.D = D; c.T = T; c.Zn = n_inducing;
    c.Z = Z; c.m = m; c.C = C; c.raw_ls = raw_lengthscale; c.raw_os = raw_outputscale; c.raw_noise = raw_noise;
    c.idx = idx; c.bb = batch_begin; c.n_idx = n_idx; c.n_steps = n_steps; c.lr = lr; c.apply = 1; c.loss_trace = loss_trace;
    return run(device, "gpt_svgp_train", c);
}

extern "C" int gpt_svgp_elbo_grad(int device, const double* Xb, const double* Yb, int64_t b, int64_t num_data, int D, int T, int n_inducing,
                                  const double* Z, const double* m, const double* C, const double* raw_lengthscale,
                                  const double* raw_outputscale, const double* raw_noise, double* loss, double* grad_Z, double* grad_m,
                                  double* grad_C, double* grad_raw_lengthscale, double* grad_raw_outputscale, double* grad_raw_noise) {
    const double* params[6] = {Z, m, C, raw_lengthscale, raw_outputscale, raw_noise};
    double* grads[6] = {grad_Z, grad_m, grad_C, grad_raw_lengthscale, grad_raw_outputscale, grad_raw_noise};
    return svgp_elbo_grad(run, "gpt_svgp_elbo_grad", SV_LIMITS, device, Xb, Yb, b, num_data, D, T, n_inducing, params, loss, grads);
}
