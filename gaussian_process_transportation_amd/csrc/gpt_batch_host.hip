// Entry points of the batch of small exact GPs — gpt_batch_lml_objective, gpt_batch_fit, gpt_batch_predict (include/gpt_hip.h):
// argument checks, the two device images of a call's inputs, the output images, the read-back and the scatter.  Host code only
// (the kernels: gpt_batch.hip, reached through the launchers of gpt_batch.h), so it also compiles under g++ against host_stub/
// and runs under the sanitizers (make host-oneshot-asan).
#include "gpt_batch.h"
#include "gpt_call.h"

#include <algorithm>

namespace gpt {

int check_batch_geometry(const std::string& w, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                         int n_ls, double jitter, int ktype) {
    if (B < 1 || B > BAT_MAX_B) return fail(GPT_E_ARG, w + ": B (models) must be 1 .. 2^20, got " + std::to_string(B));
    if (D < 1 || D > MAX_DIMS) return fail(GPT_E_ARG, w + ": D must be 1 .. 15, got " + std::to_string(D));
    if (O < 1 || O > BAT_MAX_O) return fail(GPT_E_ARG, w + ": O (outputs) must be 1 .. 16, got " + std::to_string(O));
    if (n_ls != 1 && n_ls != D) return fail(GPT_E_ARG, w + ": n_ls must be 1 or D");
    if (ktype < GPT_KERNEL_RBF || ktype > GPT_KERNEL_MATERN52) return fail(GPT_E_ARG, w + ": unknown kernel_type");
    if (!(jitter >= 0) || !std::isfinite(jitter)) return fail(GPT_E_ARG, w + ": alpha_jitter must be finite and >= 0");
    if (n_begin[0] != 0) return fail(GPT_E_ARG, w + ": n_begin[0] must be 0");
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = n_begin[b + 1] - n_begin[b];
        if (n < 1 || n > BAT_MAX_N)
            return fail(GPT_E_ARG, w + ": every model needs 1 <= n_b <= 128 points with increasing offsets; model " + std::to_string(b) +
                                       " has n_begin " + std::to_string(n_begin[b]) + " .. " + std::to_string(n_begin[b + 1]));
    }
    if (!all_finite(X, (size_t)n_begin[B] * D) || !all_finite(Y, (size_t)n_begin[B] * O))
        return fail(GPT_E_ARG, w + ": X or Y contains NaN or infinity");
    return GPT_OK;
}

int small_class_first(const int64_t* n_begin, const int* model, int64_t count, std::vector<int>& list) {
    std::vector<int> large;
    list.clear();
    list.reserve(count);
    for (int64_t i = 0; i < count; ++i) {
        const int64_t b = model ? model[i] : i;
        (n_begin[b + 1] - n_begin[b] <= BAT_SMALL_N ? list : large).push_back((int)i);
    }
    const int n_small = (int)list.size();
    list.insert(list.end(), large.begin(), large.end());
    return n_small;
}

namespace {

// What the three entry points share: the validated batch and the prefix sums the kernels index by.
struct Batch {
    int64_t B = 0, rows = 0, l_total = 0, w_total = 0;
    int n_small = 0;                      // models of the small size class; they come first in `list`
    std::vector<int64_t> l_begin, w_begin;
    std::vector<int> list;
};

int check_batch(const std::string& w, Batch& bt, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                const double* ls, int n_ls, const double* c, const double* noise, double jitter, int ktype, const int* status) {
    if (!X || !Y || !n_begin || !ls || !c || !noise || !status) return fail(GPT_E_ARG, w + ": NULL argument");
    if (int rc = check_batch_geometry(w, X, Y, n_begin, B, D, O, n_ls, jitter, ktype)) return rc;
    bt.B = B;
    bt.l_begin.assign(B + 1, 0);
    bt.w_begin.assign(B + 1, 0);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = n_begin[b + 1] - n_begin[b];
        bt.l_begin[b + 1] = bt.l_begin[b] + n * n;
        bt.w_begin[b + 1] = bt.w_begin[b] + n * (n + 1) / 2;
    }
    bt.n_small = small_class_first(n_begin, nullptr, B, bt.list);
    bt.rows = n_begin[B];
    bt.l_total = bt.l_begin[B];
    bt.w_total = bt.w_begin[B];
    for (int64_t e = 0; e < B * n_ls; ++e)
        if (!(ls[e] > 0) || !std::isfinite(ls[e])) return fail(GPT_E_ARG, w + ": length_scale must be finite and > 0 (model " + std::to_string(e / n_ls) + ")");
    for (int64_t b = 0; b < B; ++b)
        if (!(c[b] > 0) || !std::isfinite(c[b]) || !(noise[b] >= 0) || !std::isfinite(noise[b]))
            return fail(GPT_E_ARG, w + ": need finite constant_value > 0 and noise_level >= 0 (model " + std::to_string(b) + ")");
    return GPT_OK;
}

// Device image of a call's inputs: one buffer of doubles and one of integers, one copy each.
struct BatDevice {
    double *X, *Y, *ls, *c, *noise, *Xq = nullptr;
    int64_t *n_begin, *l_begin, *w_begin, *q_begin = nullptr;
    int *list, *tile_model = nullptr, *tile_q0 = nullptr;
};

int upload(CallBuffers& buf, BatDevice& dv, const Batch& bt, const double* X, const double* Y, const int64_t* n_begin, int D, int O,
           const double* ls, int n_ls, const double* c, const double* noise, const double* Xq, const int64_t* q_begin,
           const std::vector<int>& tile_model, const std::vector<int>& tile_q0) {
    const size_t B = (size_t)bt.B, nx = (size_t)bt.rows * D, ny = (size_t)bt.rows * O, nq = q_begin ? (size_t)q_begin[B] * D : 0;
    std::vector<double> hd;
    hd.reserve(nx + ny + B * (n_ls + 2) + nq);
    hd.insert(hd.end(), X, X + nx);
    hd.insert(hd.end(), Y, Y + ny);
    hd.insert(hd.end(), ls, ls + B * n_ls);
    hd.insert(hd.end(), c, c + B);
    hd.insert(hd.end(), noise, noise + B);
    if (nq) hd.insert(hd.end(), Xq, Xq + nq);
    const size_t nt = tile_model.size();
    std::vector<int64_t> hi(4 * (B + 1) + (B + 2 * nt + 1) / 2 + 1, 0);
    std::copy(n_begin, n_begin + B + 1, hi.begin());
    std::copy(bt.l_begin.begin(), bt.l_begin.end(), hi.begin() + (B + 1));
    std::copy(bt.w_begin.begin(), bt.w_begin.end(), hi.begin() + 2 * (B + 1));
    if (q_begin) std::copy(q_begin, q_begin + B + 1, hi.begin() + 3 * (B + 1));
    int* h32 = reinterpret_cast<int*>(hi.data() + 4 * (B + 1));
    std::copy(bt.list.begin(), bt.list.end(), h32);
    std::copy(tile_model.begin(), tile_model.end(), h32 + B);
    std::copy(tile_q0.begin(), tile_q0.end(), h32 + B + nt);

    double* dd;
    int64_t* di;
    CALLCHK(buf.alloc(&dd, hd.size()));
    CALLCHK(buf.alloc(&di, hi.size()));
    CALLCHK(hipMemcpyAsync(dd, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipMemcpyAsync(di, hi.data(), hi.size() * sizeof(int64_t), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));          // the staging vectors end with this function
    dv.X = dd; dv.Y = dv.X + nx; dv.ls = dv.Y + ny; dv.c = dv.ls + B * n_ls; dv.noise = dv.c + B; dv.Xq = dv.noise + B;
    dv.n_begin = di; dv.l_begin = di + (B + 1); dv.w_begin = di + 2 * (B + 1); dv.q_begin = di + 3 * (B + 1);
    dv.list = reinterpret_cast<int*>(di + 4 * (B + 1));
    dv.tile_model = dv.list + B;
    dv.tile_q0 = dv.tile_model + nt;
    return GPT_OK;
}

BatArgs factor_args(const BatDevice& dv, int D, int O, int n_ls, double jitter) {
    BatArgs a{};
    a.X = dv.X; a.Y = dv.Y; a.ls = dv.ls; a.c = dv.c; a.noise = dv.noise;
    a.n_begin = dv.n_begin; a.l_begin = dv.l_begin; a.w_begin = dv.w_begin; a.list = dv.list;
    a.D = D; a.O = O; a.n_ls = n_ls; a.jitter = jitter;
    return a;
}

// dst[begin[b] * width ..] = src[...] for every model whose status is GPT_OK (a failed model's outputs stay untouched)
void scatter_ok(double* dst, const double* src, const int64_t* begin, size_t width, const int* status, int64_t B) {
    if (!dst) return;
    for (int64_t b = 0; b < B; ++b)
        if (status[b] == GPT_OK)
            std::copy(src + (size_t)begin[b] * width, src + (size_t)begin[b + 1] * width, dst + (size_t)begin[b] * width);
}

}  // namespace
}  // namespace gpt

using namespace gpt;

extern "C" int gpt_batch_lml_objective(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                                       const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                                       double alpha_jitter, int kernel_type, double* lml, double* grad, int* status) {
    const std::string w = "gpt_batch_lml_objective";
    if (!lml || !grad) return fail(GPT_E_ARG, w + ": NULL argument");
    Batch bt;
    if (int rc = check_batch(w, bt, X, Y, n_begin, B, D, O, length_scale, n_ls, constant_value, noise_level, alpha_jitter, kernel_type, status))
        return rc;
    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    BatDevice dv;
    if (int rc = upload(buf, dv, bt, X, Y, n_begin, D, O, length_scale, n_ls, constant_value, noise_level, nullptr, nullptr, {}, {})) return rc;
    const size_t G = 2 + n_ls, nout = (size_t)B * (1 + G) + ((size_t)B + 1) / 2;      // lml | grad | status (int)
    double* dout;
    CALLCHK(buf.alloc(&dout, nout));
    BatArgs a = factor_args(dv, D, O, n_ls, alpha_jitter);
    a.lml = dout; a.grad = dout + B; a.status = reinterpret_cast<int*>(dout + (size_t)B * (1 + G));
    launch_bat_factor(buf.stream, kernel_type, true, bt.n_small, (int)(bt.B - bt.n_small), a);
    CALLCHK(hipGetLastError());
    std::vector<double> out(nout);
    CALLCHK(hipMemcpyAsync(out.data(), dout, nout * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));
    const int* st = reinterpret_cast<const int*>(out.data() + (size_t)B * (1 + G));
    for (int64_t b = 0; b < B; ++b) {
        status[b] = st[b];
        if (st[b] != GPT_OK) continue;
        lml[b] = out[b];
        std::copy(out.begin() + B + b * G, out.begin() + B + (b + 1) * G, grad + b * G);
    }
    return GPT_OK;
}

extern "C" int gpt_batch_fit(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                             const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                             double alpha_jitter, int kernel_type, double* L, double* alpha, double* lml, int* status) {
    const std::string w = "gpt_batch_fit";
    if (!alpha) return fail(GPT_E_ARG, w + ": NULL argument");
    Batch bt;
    if (int rc = check_batch(w, bt, X, Y, n_begin, B, D, O, length_scale, n_ls, constant_value, noise_level, alpha_jitter, kernel_type, status))
        return rc;
    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    BatDevice dv;
    if (int rc = upload(buf, dv, bt, X, Y, n_begin, D, O, length_scale, n_ls, constant_value, noise_level, nullptr, nullptr, {}, {})) return rc;
    const size_t na = (size_t)bt.rows * O, nl = L ? (size_t)bt.l_total : 0, nout = (size_t)B + na + nl + ((size_t)B + 1) / 2;
    double* dout;                                                                     // lml | alpha | L | status (int)
    CALLCHK(buf.alloc(&dout, nout));
    BatArgs a = factor_args(dv, D, O, n_ls, alpha_jitter);
    a.lml = dout; a.alpha = dout + B; a.L = L ? dout + B + na : nullptr; a.status = reinterpret_cast<int*>(dout + B + na + nl);
    launch_bat_factor(buf.stream, kernel_type, false, bt.n_small, (int)(bt.B - bt.n_small), a);
    CALLCHK(hipGetLastError());
    std::vector<double> out(nout);
    CALLCHK(hipMemcpyAsync(out.data(), dout, nout * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));
    const int* st = reinterpret_cast<const int*>(out.data() + B + na + nl);
    std::copy(st, st + B, status);
    if (lml)
        for (int64_t b = 0; b < B; ++b)
            if (st[b] == GPT_OK) lml[b] = out[b];
    scatter_ok(alpha, out.data() + B, n_begin, O, st, B);
    scatter_ok(L, out.data() + B + na, bt.l_begin.data(), 1, st, B);
    return GPT_OK;
}

extern "C" int gpt_batch_predict(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                                 const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                                 double alpha_jitter, int kernel_type, const double* Xq, const int64_t* q_begin, double* mean, double* var,
                                 double* J, double* Jvar, double* dvar, int* status) {
    const std::string w = "gpt_batch_predict";
    if (!q_begin) return fail(GPT_E_ARG, w + ": NULL argument");
    Batch bt;
    if (int rc = check_batch(w, bt, X, Y, n_begin, B, D, O, length_scale, n_ls, constant_value, noise_level, alpha_jitter, kernel_type, status))
        return rc;
    const bool der = J || Jvar || dvar;
    if (der && kernel_type != GPT_KERNEL_RBF)
        return fail(GPT_E_ARG, w + ": J, Jvar and dvar are RBF only in a batch (the analytic Matern derivatives: GaussianProcess(matern_derivatives=True))");
    if (q_begin[0] != 0) return fail(GPT_E_ARG, w + ": q_begin[0] must be 0");
    for (int64_t b = 0; b < B; ++b)
        if (q_begin[b + 1] < q_begin[b] || q_begin[b + 1] > INT_MAX)
            return fail(GPT_E_ARG, w + ": q_begin must not decrease (M_b >= 0) and the queries of a call must number fewer than 2^31 (model " +
                                       std::to_string(b) + ")");
    const int64_t M = q_begin[B];
    if (M > 0 && !Xq) return fail(GPT_E_ARG, w + ": NULL argument");
    if (M > 0 && !all_finite(Xq, (size_t)M * D)) return fail(GPT_E_ARG, w + ": Xq contains NaN or infinity");
    // tiles of 64 queries, in the order of bt.list: the small size class first
    std::vector<int> tile_model, tile_q0;
    int tiles_small = 0;
    for (int64_t k = 0; k < B; ++k) {
        const int b = bt.list[k];
        for (int64_t q0 = 0; q0 < q_begin[b + 1] - q_begin[b]; q0 += BAT_QT) { tile_model.push_back(b); tile_q0.push_back((int)q0); }
        if (k + 1 == bt.n_small) tiles_small = (int)tile_model.size();
    }
    if (bt.n_small == 0) tiles_small = 0;
    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    BatDevice dv;
    if (int rc = upload(buf, dv, bt, X, Y, n_begin, D, O, length_scale, n_ls, constant_value, noise_level, Xq, q_begin, tile_model, tile_q0))
        return rc;
    // scratch of the factor: alpha | packed W | status; then the outputs asked for
    const size_t na = (size_t)bt.rows * O;
    double *dfac, *dout;
    CALLCHK(buf.alloc(&dfac, na + (size_t)bt.w_total + ((size_t)B + 1) / 2));
    const size_t widths[5] = {mean ? (size_t)O : 0, var ? (size_t)1 : 0, J ? (size_t)O * D : 0, Jvar ? (size_t)D : 0, dvar ? (size_t)D : 0};
    size_t off[6] = {0};
    for (int k = 0; k < 5; ++k) off[k + 1] = off[k] + widths[k] * (size_t)M;
    CALLCHK(buf.alloc(&dout, off[5]));
    BatArgs a = factor_args(dv, D, O, n_ls, alpha_jitter);
    a.alpha = dfac; a.Wp = dfac + na; a.status = reinterpret_cast<int*>(dfac + na + bt.w_total);
    launch_bat_factor(buf.stream, kernel_type, false, bt.n_small, (int)(bt.B - bt.n_small), a);
    BatPredArgs p{};
    p.X = dv.X; p.ls = dv.ls; p.c = dv.c; p.noise = dv.noise; p.alpha = a.alpha; p.Wp = a.Wp; p.Xq = dv.Xq;
    p.n_begin = dv.n_begin; p.w_begin = dv.w_begin; p.q_begin = dv.q_begin; p.tile_model = dv.tile_model; p.tile_q0 = dv.tile_q0;
    p.status = a.status; p.D = D; p.O = O; p.n_ls = n_ls;
    p.mean = mean ? dout + off[0] : nullptr; p.var = var ? dout + off[1] : nullptr; p.J = J ? dout + off[2] : nullptr;
    p.Jvar = Jvar ? dout + off[3] : nullptr; p.dvar = dvar ? dout + off[4] : nullptr;
    if (off[5] > 0) launch_bat_predict(buf.stream, kernel_type, der, tiles_small, (int)tile_model.size() - tiles_small, p);
    CALLCHK(hipGetLastError());
    std::vector<double> out(off[5]);
    std::vector<int> st(B);
    CALLCHK(hipMemcpyAsync(st.data(), a.status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, buf.stream));
    if (off[5] > 0) CALLCHK(hipMemcpyAsync(out.data(), dout, off[5] * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));
    std::copy(st.begin(), st.end(), status);
    double* dst[5] = {mean, var, J, Jvar, dvar};
    for (int k = 0; k < 5; ++k) scatter_ok(dst[k], out.data() + off[k], q_begin, widths[k], st.data(), B);
    return GPT_OK;
}
