// Entry point of the fold scan of a batch of small displacement maps — gpt_batch_fold_scan (include/gpt_hip.h): argument checks,
// the surrogate's inputs, the tiles, the device images of the call, the three launches, the read-back and the scatter.  Host code
// only (the kernels: gpt_fold_scan.hip, reached through the launchers of gpt_fold_scan.h), so it also compiles under g++ against
// host_stub/ and runs under the sanitizers (make host-oneshot-asan).
#include "gpt_fold_scan.h"
#include "gpt_call.h"

#include <algorithm>

using namespace gpt;

extern "C" int gpt_batch_fold_scan(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D,
                                   const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                                   double alpha_jitter, int kernel_type, const double* Xq, const int64_t* q_begin, int64_t M, int surrogate,
                                   double* min_det, int64_t* argmin, int64_t* n_fold, double* err_sum, double* err_max, double* det, double* z,
                                   double* err, int* status, int* surrogate_status) {
    const std::string w = "gpt_batch_fold_scan";
    if (!X || !Y || !n_begin || !length_scale || !constant_value || !noise_level || !min_det || !argmin || !n_fold || !status)
        return fail(GPT_E_ARG, w + ": NULL argument");
    if (surrogate && (!err_sum || !err_max || !surrogate_status))
        return fail(GPT_E_ARG, w + ": NULL argument (err_sum, err_max and surrogate_status are needed with the surrogate)");
    if (D < 1 || D > FS_MAX_D)
        return fail(GPT_E_ARG, w + ": D must be 1 .. 3 (the map x -> x + psi(x) is a displacement: O = D <= 3), got " + std::to_string(D));
    if (kernel_type != GPT_KERNEL_RBF)
        return fail(GPT_E_ARG, w + ": RBF only (the batch family has no Matern derivatives: gpt_batch_predict refuses J of a Matern batch too)");
    if (int rc = check_batch_geometry(w, X, Y, n_begin, B, D, D, n_ls, alpha_jitter, kernel_type)) return rc;
    for (int64_t e = 0; e < B * n_ls; ++e)
        if (!(length_scale[e] > 0) || !std::isfinite(length_scale[e]))
            return fail(GPT_E_ARG, w + ": length_scale must be finite and > 0 (model " + std::to_string(e / n_ls) + ")");
    for (int64_t b = 0; b < B; ++b)
        if (!(constant_value[b] > 0) || !std::isfinite(constant_value[b]) || !(noise_level[b] >= 0) || !std::isfinite(noise_level[b]))
            return fail(GPT_E_ARG, w + ": need finite constant_value > 0 and noise_level >= 0 (model " + std::to_string(b) + ")");

    // where a model's per-query outputs begin; the queries themselves are shared (q_begin null) or ragged by the same offsets
    const bool shared = q_begin == nullptr;
    std::vector<int64_t> o_begin((size_t)B + 1, 0);
    if (shared) {
        if (M < 0 || M > INT_MAX / B)
            return fail(GPT_E_ARG, w + ": M must be >= 0 and the queries of a call (B M) must number fewer than 2^31, got M = " + std::to_string(M));
        for (int64_t b = 0; b <= B; ++b) o_begin[b] = b * M;
    } else {
        if (q_begin[0] != 0) return fail(GPT_E_ARG, w + ": q_begin[0] must be 0");
        for (int64_t b = 0; b < B; ++b)
            if (q_begin[b + 1] < q_begin[b] || q_begin[b + 1] > INT_MAX)
                return fail(GPT_E_ARG, w + ": q_begin must not decrease (M_b >= 0) and the queries of a call must number fewer than 2^31 (model " +
                                           std::to_string(b) + ")");
        std::copy(q_begin, q_begin + B + 1, o_begin.begin());
    }
    const size_t Mq = shared ? (size_t)M : (size_t)q_begin[B], Mo = (size_t)o_begin[B];    // rows of Xq; rows of det, z, err
    if (Mq > 0 && !Xq) return fail(GPT_E_ARG, w + ": NULL argument");
    if (Mq > 0 && !all_finite(Xq, Mq * D)) return fail(GPT_E_ARG, w + ": Xq contains NaN or infinity");

    // tiles of BAT_QT queries in the order of the launch list: the small size class first, a model's tiles together
    std::vector<int> list, tile_model, tile_q0, tile_first((size_t)B, 0);
    const int n_small = small_class_first(n_begin, nullptr, B, list);
    int tiles_small = 0;
    for (int64_t k = 0; k < B; ++k) {
        const int b = list[k];
        tile_first[b] = (int)tile_model.size();
        for (int64_t q0 = 0; q0 < o_begin[b + 1] - o_begin[b]; q0 += BAT_QT) { tile_model.push_back(b); tile_q0.push_back((int)q0); }
        if (k + 1 == n_small) tiles_small = (int)tile_model.size();
    }
    const size_t nt = tile_model.size();

    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    // doubles in:   X | Y | Xs = X + Y | Ys = -Y (the last two with the surrogate) | ls | c | noise | Xq
    // integers in:  n_begin | o_begin (int64) | list | tile_first | tile_model | tile_q0 (int)
    const size_t rows = (size_t)n_begin[B], nx = rows * D, ns = surrogate ? nx : 0, nh = (size_t)B * (n_ls + 2), nq = Mq * D;
    std::vector<double> hd;
    hd.reserve(2 * nx + 2 * ns + nh + nq);
    hd.insert(hd.end(), X, X + nx);
    hd.insert(hd.end(), Y, Y + nx);
    for (size_t e = 0; e < ns; ++e) hd.push_back(X[e] + Y[e]);           // the reference's target_distribution (:117)
    for (size_t e = 0; e < ns; ++e) hd.push_back(-Y[e]);                 // delta_inv (:115)
    hd.insert(hd.end(), length_scale, length_scale + (size_t)B * n_ls);
    hd.insert(hd.end(), constant_value, constant_value + B);
    hd.insert(hd.end(), noise_level, noise_level + B);
    if (nq) hd.insert(hd.end(), Xq, Xq + nq);
    std::vector<int64_t> hi(2 * ((size_t)B + 1) + (2 * (size_t)B + 2 * nt + 1) / 2, 0);
    std::copy(n_begin, n_begin + B + 1, hi.begin());
    std::copy(o_begin.begin(), o_begin.end(), hi.begin() + (B + 1));
    int* h32 = reinterpret_cast<int*>(hi.data() + 2 * (B + 1));
    std::copy(list.begin(), list.end(), h32);
    std::copy(tile_first.begin(), tile_first.end(), h32 + B);
    std::copy(tile_model.begin(), tile_model.end(), h32 + 2 * B);
    std::copy(tile_q0.begin(), tile_q0.end(), h32 + 2 * B + nt);
    double* dd;
    int64_t* di;
    CALLCHK(buf.alloc(&dd, hd.size()));
    CALLCHK(buf.alloc(&di, hi.size()));
    CALLCHK(hipMemcpyAsync(dd, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipMemcpyAsync(di, hi.data(), hi.size() * sizeof(int64_t), hipMemcpyHostToDevice, buf.stream));

    // work:     alpha | beta | tile partials (doubles); tile partials (ints)
    // outputs:  min_det | err_sum | err_max (B each) | det | z | err (those asked for);  argmin | n_fold (int64) | status | surrogate status (int)
    const size_t widths[3] = {det ? (size_t)1 : 0, z ? (size_t)D : 0, (err && surrogate) ? (size_t)1 : 0};
    size_t off[4] = {3 * (size_t)B, 0, 0, 0};
    for (int k = 0; k < 3; ++k) off[k + 1] = off[k] + widths[k] * Mo;
    double *dwork, *dout;
    int64_t* dio;
    int* dip;
    CALLCHK(buf.alloc(&dwork, nx + ns + nt * FS_PART_D));
    CALLCHK(buf.alloc(&dip, nt * FS_PART_I));
    CALLCHK(buf.alloc(&dout, off[3]));
    CALLCHK(buf.alloc(&dio, 3 * (size_t)B));

    FoldScanArgs a{};
    a.X = dd; a.Y = dd + nx; a.Xs = surrogate ? dd + 2 * nx : nullptr; a.Ys = surrogate ? dd + 2 * nx + ns : nullptr;
    a.ls = dd + 2 * nx + 2 * ns; a.c = a.ls + (size_t)B * n_ls; a.noise = a.c + B; a.Xq = a.noise + B;
    a.n_begin = di; a.o_begin = di + (B + 1);
    a.list = reinterpret_cast<int*>(di + 2 * (B + 1)); a.tile_first = a.list + B; a.tile_model = a.list + 2 * B; a.tile_q0 = a.tile_model + nt;
    a.alpha = dwork; a.beta = surrogate ? dwork + nx : nullptr; a.part = dwork + nx + ns; a.ipart = dip;
    a.min_det = dout; a.err_sum = dout + B; a.err_max = dout + 2 * B;
    a.det = widths[0] ? dout + off[0] : nullptr; a.z = widths[1] ? dout + off[1] : nullptr; a.err = widths[2] ? dout + off[2] : nullptr;
    a.argmin = dio; a.n_fold = dio + B;
    a.status = reinterpret_cast<int*>(dio + 2 * B); a.sur_status = surrogate ? a.status + B : nullptr;
    a.D = D; a.n_ls = n_ls; a.shared = shared; a.surrogate = surrogate != 0; a.jitter = alpha_jitter;

    launch_fs_factor(buf.stream, n_small, (int)(B - n_small), a);
    launch_fs_scan(buf.stream, tiles_small, (int)nt - tiles_small, B, a);
    CALLCHK(hipGetLastError());
    std::vector<double> out(off[3]);
    std::vector<int64_t> outi(3 * (size_t)B);
    CALLCHK(hipMemcpyAsync(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipMemcpyAsync(outi.data(), dio, outi.size() * sizeof(int64_t), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));

    // a model that is not PD keeps all of its outputs; one whose surrogate alone is not PD keeps its err outputs
    const int* st = reinterpret_cast<const int*>(outi.data() + 2 * B);
    double* dst[3] = {det, z, err};
    for (int64_t b = 0; b < B; ++b) {
        status[b] = st[b];
        if (st[b] != GPT_OK) continue;
        min_det[b] = out[b];
        argmin[b] = outi[b];
        n_fold[b] = outi[B + b];
        const bool sur_ok = surrogate && st[B + b] == GPT_OK;
        if (surrogate) surrogate_status[b] = st[B + b];
        if (sur_ok) { err_sum[b] = out[B + b]; err_max[b] = out[2 * B + b]; }
        for (int k = 0; k < 3; ++k)
            if (widths[k] && (k < 2 || sur_ok))
                std::copy(out.begin() + off[k] + (size_t)o_begin[b] * widths[k], out.begin() + off[k] + (size_t)o_begin[b + 1] * widths[k],
                          dst[k] + (size_t)o_begin[b] * widths[k]);
    }
    return GPT_OK;
}
