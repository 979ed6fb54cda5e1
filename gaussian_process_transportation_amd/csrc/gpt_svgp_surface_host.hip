// gpt_svgp_surface_train, gpt_svgp_surface_elbo_grad and gpt_svgp_surface_predict (include/gpt_hip.h): argument checks, the flat
// theta layout packed on the way in and scattered on the way out, the workspace of a call, the per-task host images of the
// prediction, the read-back.  Host code only (the kernels: gpt_svgp_surface.hip, reached through the launchers of
// gpt_svgp_surface.h), so it also compiles under g++ against host_stub/ and runs under the sanitizers (make host-oneshot-asan).
#include "gpt_svgp_surface.h"

using namespace gpt;

namespace {

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

double host_softplus(double x) { return x > 20.0 ? x : std::log1p(std::exp(x)); }

int run(int device, const char* who, const SvgpCall& c) {
    const std::string w = who;
    int bmax = 0;
    if (int rc = svgp_validate(w, c, SF_LIMITS, (size_t)c.T * c.D, &bmax)) return rc;
    if (int rc = use_device(w, device)) return rc;
    const int D = c.D, T = c.T, Zn = c.Zn;

    const int NP = (int)round_up(Zn, PAD_N), BP = (int)round_up(bmax, 64);
    const int64_t ZZ = (int64_t)Zn * Zn, NN = (int64_t)NP * NP, NB_ = (int64_t)NP * BP;
    const int64_t nz = (int64_t)Zn * D, SH = round_up(nz + 1, 64), task_stride = SF_HDR + NP + NN, n_theta = SH + T * task_stride;
    std::vector<double> th(n_theta, 0.0);
    for (int64_t e = 0; e < nz; ++e) th[e] = c.Z[e];
    th[nz] = c.raw_noise[T];
    for (int t = 0; t < T; ++t) {
        double* p = th.data() + SH + t * task_stride;
        p[0] = c.raw_os[t];
        p[1] = c.raw_noise[t];
        for (int d = 0; d < D; ++d) p[2 + d] = c.raw_ls[t * D + d];
        for (int i = 0; i < Zn; ++i) p[SF_HDR + i] = c.m[(int64_t)t * Zn + i];
        for (int i = 0; i < Zn; ++i)
            for (int j = 0; j <= i; ++j) p[SF_HDR + NP + (int64_t)i * NP + j] = c.C[t * ZZ + (int64_t)i * Zn + j];   // the strict upper triangle is not a parameter
    }
    std::vector<int> idx32;
    CallBuffers buf;
    CALLCHK(buf.open());
    const hipStream_t s = buf.stream;
    SvgpDevice dev;
    if (int rc = svgp_upload(buf, c, th, &idx32, &dev)) return rc;
    SfArgs a{};
    a.X = dev.X; a.Y = dev.Y; a.idx = dev.idx; a.loss = dev.loss; a.fail = dev.fail;
    a.theta = dev.theta; a.grad = dev.grad; a.m1 = dev.m1; a.m2 = dev.m2;
    a.N = (int)c.N; a.D = D; a.T = T; a.Zn = Zn; a.NP = NP; a.BP = BP; a.num_data = (double)c.num_data;
    a.SH = SH; a.task_stride = task_stride; a.part_stride = 2 + nz;
    CALLCHK(buf.alloc(&a.part, (size_t)T * a.part_stride));
    for (double** p : {&a.K, &a.W, &a.Q, &a.M2}) CALLCHK(buf.alloc(p, (size_t)NN));
    for (double** p : {&a.Kx, &a.A, &a.U, &a.CU, &a.Ab, &a.B}) CALLCHK(buf.alloc(p, (size_t)NB_));
    CALLCHK(buf.alloc(&a.scr, factor_scratch_doubles(NP)));
    CALLCHK(buf.alloc(&a.stat, (size_t)3 * BP));
    CALLCHK(buf.alloc(&a.rbuf, (size_t)BP));
    CALLCHK(buf.alloc(&a.klrow, (size_t)NP));
    CALLCHK(buf.alloc(&a.rowpart, (size_t)NP * (1 + D)));
    CALLCHK(buf.alloc(&a.sc, 8));
    CALLCHK(buf.alloc(&a.info, (size_t)T));
    CALLCHK(hipMemsetAsync(a.grad, 0, (size_t)n_theta * 8, s));
    CALLCHK(hipMemsetAsync(a.info, 0, (size_t)T * sizeof(int), s));

    launch_sf_train(s, a, c.bb, c.n_steps, c.apply, c.lr);
    std::vector<double> out(n_theta);
    double* dst[6];
    if (int rc = svgp_read_back(w, s, c, dev, &out, dst)) return rc;
    if (dst[0]) for (int64_t e = 0; e < nz; ++e) dst[0][e] = out[e];
    if (dst[5]) dst[5][T] = out[nz];
    for (int t = 0; t < T; ++t) {
        const double* p = out.data() + SH + t * task_stride;
        if (dst[4]) dst[4][t] = p[0];
        if (dst[5]) dst[5][t] = p[1];
        if (dst[3]) for (int d = 0; d < D; ++d) dst[3][t * D + d] = p[2 + d];
        if (dst[1]) for (int i = 0; i < Zn; ++i) dst[1][(int64_t)t * Zn + i] = p[SF_HDR + i];
        if (dst[2])
            for (int i = 0; i < Zn; ++i)
                for (int j = 0; j < Zn; ++j)
                    if (j <= i || !c.apply) dst[2][t * ZZ + (int64_t)i * Zn + j] = j <= i ? p[SF_HDR + NP + (int64_t)i * NP + j] : 0.0;
    }
    return GPT_OK;
}

}  // namespace

extern "C" int gpt_svgp_surface_train(int device, const double* X, const double* Y, int64_t N, int D, int T, int n_inducing, double* Z,
                                      double* m, double* C, double* raw_lengthscale, double* raw_outputscale, double* raw_noise,
                                      const int64_t* idx, int64_t n_idx, const int64_t* batch_begin, int64_t n_steps, double lr,
                                      double* loss_trace) {
    SvgpCall c{};
    c.X = X; c.Y = Y; c.N = N; c.num_data = N; c.D = D; c.T = T; c.Zn = n_inducing;
    c.Z = Z; c.m = m; c.C = C; c.raw_ls = raw_lengthscale; c.raw_os = raw_outputscale; c.raw_noise = raw_noise;
    c.idx = idx; c.bb = batch_begin; c.n_idx = n_idx; c.n_steps = n_steps; c.lr = lr; c.apply = 1; c.loss_trace = loss_trace;
    return run(device, "gpt_svgp_surface_train", c);
}

extern "C" int gpt_svgp_surface_elbo_grad(int device, const double* Xb, const double* Yb, int64_t b, int64_t num_data, int D, int T,
                                          int n_inducing, const double* Z, const double* m, const double* C, const double* raw_lengthscale,
                                          const double* raw_outputscale, const double* raw_noise, double* loss, double* grad_Z,
                                          double* grad_m, double* grad_C, double* grad_raw_lengthscale, double* grad_raw_outputscale,
                                          double* grad_raw_noise) {
    const double* params[6] = {Z, m, C, raw_lengthscale, raw_outputscale, raw_noise};
    double* grads[6] = {grad_Z, grad_m, grad_C, grad_raw_lengthscale, grad_raw_outputscale, grad_raw_noise};
    return svgp_elbo_grad(run, "gpt_svgp_surface_elbo_grad", SF_LIMITS, device, Xb, Yb, b, num_data, D, T, n_inducing, params, loss, grads);
}

extern "C" int gpt_svgp_surface_predict(int device, const double* Z, const double* m, const double* C, const double* raw_lengthscale,
                                        const double* raw_outputscale, int n_inducing, int D, int T, const double* Xq, int64_t M,
                                        double* mean, double* var, double* J) {
    const std::string w = "gpt_svgp_surface_predict";
    if (!Z || !m || !C || !raw_lengthscale || !raw_outputscale || !Xq || !mean) return fail(GPT_E_ARG, w + ": NULL argument");
    const int Zn = n_inducing;
    if (int rc = svgp_check_model(w, SF_LIMITS, D, T, Zn)) return rc;
    if (M < 1 || M > ((int64_t)1 << 40)) return fail(GPT_E_ARG, w + ": M (queries) must be >= 1");
    const int64_t ZZ = (int64_t)Zn * Zn;
    if (!all_finite(Z, (size_t)Zn * D) || !all_finite(m, (size_t)T * Zn) || !all_finite(C, (size_t)T * ZZ) ||
        !all_finite(raw_lengthscale, (size_t)T * D) || !all_finite(raw_outputscale, T) || !all_finite(Xq, (size_t)M * D))
        return fail(GPT_E_ARG, w + ": non-finite input");
    if (int rc = use_device(w, device)) return rc;
    const int NP = (int)round_up(Zn, PAD_N);
    const int MC = (int)(M < SF_PRED_CHUNK ? round_up(M, 64) : SF_PRED_CHUNK);
    const int64_t NN = (int64_t)NP * NP, NM = (int64_t)NP * MC;

    CallBuffers buf;
    CALLCHK(buf.open());
    const hipStream_t s = buf.stream;
    double *dZ, *dX, *dK, *dW, *dC, *dm, *dbeta, *dKq, *dAq, *dVq, *dscr, *dil, *dmean, *dvar = nullptr, *dJ = nullptr;
    int* dinfo;
    CALLCHK(buf.alloc(&dZ, (size_t)Zn * D));
    CALLCHK(buf.alloc(&dX, (size_t)M * D));
    CALLCHK(buf.alloc(&dK, (size_t)NN));
    CALLCHK(buf.alloc(&dW, (size_t)NN));
    CALLCHK(buf.alloc(&dC, (size_t)NN));
    CALLCHK(buf.alloc(&dm, (size_t)NP));
    CALLCHK(buf.alloc(&dbeta, (size_t)NP));
    CALLCHK(buf.alloc(&dKq, (size_t)NM));
    CALLCHK(buf.alloc(&dAq, (size_t)NM));
    CALLCHK(buf.alloc(&dVq, (size_t)NM));
    CALLCHK(buf.alloc(&dscr, factor_scratch_doubles(NP)));
    CALLCHK(buf.alloc(&dil, (size_t)MAX_D));
    CALLCHK(buf.alloc(&dinfo, 1));
    CALLCHK(buf.alloc(&dmean, (size_t)M * T));
    if (var) CALLCHK(buf.alloc(&dvar, (size_t)M * T));
    if (J) CALLCHK(buf.alloc(&dJ, (size_t)M * T * D));
    CALLCHK(hipMemcpyAsync(dZ, Z, (size_t)Zn * D * 8, hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(dX, Xq, (size_t)M * D * 8, hipMemcpyHostToDevice, s));

    SfPredArgs p{};
    p.Z = dZ; p.Xq = dX; p.K = dK; p.W = dW; p.C = dC; p.m = dm; p.il = dil; p.beta = dbeta; p.Kq = dKq; p.Aq = dAq; p.Vq = dVq;
    p.scr = dscr; p.info = dinfo; p.mean = dmean; p.var = dvar; p.J = dJ; p.Zn = Zn; p.D = D; p.T = T; p.NP = NP; p.MC = MC; p.M = M;

    std::vector<double> Kh(NN), Ch(NN), mh(NP), il(MAX_D, 0.0);
    for (int t = 0; t < T; ++t) {
        const double c = host_softplus(raw_outputscale[t]);
        for (int d = 0; d < D; ++d) il[d] = 1.0 / host_softplus(raw_lengthscale[t * D + d]);
        // K = c k(Z,Z) + eps I with identity in the padding (host: O(Z^2 D), once per task and call), C padded, m padded
        for (int64_t e = 0; e < NN; ++e) { Kh[e] = 0.0; Ch[e] = 0.0; }
        for (int i = 0; i < NP; ++i) {
            mh[i] = i < Zn ? m[(int64_t)t * Zn + i] : 0.0;
            if (i >= Zn) { Kh[(int64_t)i * NP + i] = 1.0; continue; }
            for (int j = 0; j <= i; ++j) {
                double q = 0.0;
                for (int d = 0; d < D; ++d) { const double u = (Z[i * D + d] - Z[j * D + d]) * il[d]; q += u * u; }
                const double v = c * std::exp(-0.5 * q) + (i == j ? JITTER : 0.0);
                Kh[(int64_t)i * NP + j] = v;
                Kh[(int64_t)j * NP + i] = v;
                Ch[(int64_t)i * NP + j] = C[t * ZZ + (int64_t)i * Zn + j];
            }
        }
        CALLCHK(hipMemcpyAsync(dK, Kh.data(), (size_t)NN * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemcpyAsync(dC, Ch.data(), (size_t)NN * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemcpyAsync(dm, mh.data(), (size_t)NP * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemcpyAsync(dil, il.data(), (size_t)MAX_D * 8, hipMemcpyHostToDevice, s));
        CALLCHK(hipMemsetAsync(dW, 0, (size_t)NN * 8, s));
        CALLCHK(hipMemsetAsync(dinfo, 0, sizeof(int), s));
        launch_sf_pred_factor(s, p);
        int info = 0;
        CALLCHK(hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, s));
        CALLCHK(hipStreamSynchronize(s));
        if (info != 0)
            return fail(GPT_E_NOT_PD, w + ": non-positive pivot " + std::to_string(info) + " in chol(c_t k(Z,Z) + eps I) of task " + std::to_string(t));
        launch_sf_pred_chunks(s, p, t, c);
        CALLCHK(hipGetLastError());
        CALLCHK(hipStreamSynchronize(s));       // the host images are rewritten for the next task
    }
    CALLCHK(hipMemcpyAsync(mean, dmean, (size_t)M * T * 8, hipMemcpyDeviceToHost, s));
    if (var) CALLCHK(hipMemcpyAsync(var, dvar, (size_t)M * T * 8, hipMemcpyDeviceToHost, s));
    if (J) CALLCHK(hipMemcpyAsync(J, dJ, (size_t)M * T * D * 8, hipMemcpyDeviceToHost, s));
    CALLCHK(hipStreamSynchronize(s));
    return GPT_OK;
}
