// Entry points of the device hyper-parameter search of a batch of small GPs — gpt_batch_optimize and gpt_batch_optimize_bounded,
// which gives every run bounds of its own (include/gpt_hip.h): argument
// checks, the device images of the call, the relaunch loop over the runs still live, the read-back.  Host code only (the kernel:
// gpt_batch_opt.hip, reached through the launcher of gpt_batch_opt.h), so it also compiles under g++ against host_stub/ and runs
// under the sanitizers (make host-oneshot-asan).
#include "gpt_batch_opt.h"
#include "gpt_call.h"

#include <algorithm>

using namespace gpt;

namespace {

// Both entry points: `bounds` holds one box (per_run false: every run reads it, stride 0) or one per run (per_run true: run r reads
// bounds + r * 2 P).  The checks of a box (finite, lo <= hi) and the clip of a run's start are made box by box either way.
int batch_optimize(const std::string& w, bool per_run, int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D,
                   int O, int n_ls, const int* run_model, const double* theta0, int64_t R, const double* bounds, double alpha_jitter,
                   int kernel_type, double pgtol, double ftol, int max_iter, int max_evals, int evals_per_launch, double* theta, double* lml,
                   int* iterations, int* evaluations, int* status) {
    if (!X || !Y || !n_begin || !run_model || !theta0 || !bounds || !theta || !lml || !iterations || !evaluations || !status)
        return fail(GPT_E_ARG, w + ": NULL argument");
    if (R < 1 || R > BAT_OPT_MAX_R) return fail(GPT_E_ARG, w + ": R (runs) must be 1 .. 2^20, got " + std::to_string(R));
    if (!(pgtol > 0) || !(ftol > 0) || !std::isfinite(pgtol) || !std::isfinite(ftol))
        return fail(GPT_E_ARG, w + ": pgtol and ftol must be finite and > 0");
    if (max_iter < 1 || max_evals < 1 || evals_per_launch < 1)
        return fail(GPT_E_ARG, w + ": max_iter, max_evals and evals_per_launch must be >= 1");
    if (int rc = check_batch_geometry(w, X, Y, n_begin, B, D, O, n_ls, alpha_jitter, kernel_type)) return rc;
    const size_t rows = (size_t)n_begin[B], P = 2 + (size_t)n_ls, nx = rows * D, ny = rows * O;
    const size_t boxes = per_run ? (size_t)R : 1, nb = boxes * 2 * P, bstride = per_run ? 2 * P : 0;
    if (!all_finite(bounds, nb) || !all_finite(theta0, (size_t)R * P))
        return fail(GPT_E_ARG, w + ": bounds or theta0 contains NaN or infinity");
    for (size_t k = 0; k < boxes; ++k)
        for (size_t i = 0; i < P; ++i)
            if (bounds[(k * P + i) * 2] > bounds[(k * P + i) * 2 + 1])
                return fail(GPT_E_ARG, w + ": bounds need lo <= hi (component " + std::to_string(i) + (per_run ? ", run " + std::to_string(k) : "") + ")");
    for (int64_t r = 0; r < R; ++r)
        if (run_model[r] < 0 || run_model[r] >= B) return fail(GPT_E_ARG, w + ": run_model must be 0 .. B - 1 (run " + std::to_string(r) + ")");
    // the runs of this call, the small size class first; a run's class is its model's
    std::vector<int> live;
    int n_small = small_class_first(n_begin, run_model, R, live);

    if (int rc = use_device(w, device)) return rc;
    CallBuffers buf;
    CALLCHK(buf.open());
    // doubles: X | Y | bounds (one box, or one per run) | theta (the clipped starts, then the results) | lml | records
    // ints:    n_begin (int64) | run_model | list | status | iterations | evaluations | counters
    const size_t rec = bat_opt_record((int)P), nin = nx + ny + nb + (size_t)R * P;
    std::vector<double> hd;
    hd.reserve(nin);
    hd.insert(hd.end(), X, X + nx);
    hd.insert(hd.end(), Y, Y + ny);
    hd.insert(hd.end(), bounds, bounds + nb);
    for (int64_t r = 0; r < R; ++r) {
        const double* bd = bounds + (size_t)r * bstride;
        for (size_t i = 0; i < P; ++i) hd.push_back(std::min(std::max(theta0[r * P + i], bd[2 * i]), bd[2 * i + 1]));
    }
    double* dd;
    int64_t* dnb;
    int* di;
    CALLCHK(buf.alloc(&dd, nin + (size_t)R + (size_t)R * rec));
    CALLCHK(buf.alloc(&dnb, (size_t)B + 1));
    CALLCHK(buf.alloc(&di, (size_t)R * (5 + BAT_OPT_CNT)));
    BatOptArgs a{};
    a.X = dd; a.Y = dd + nx; a.bounds = dd + nx + ny; a.bounds_stride = (int64_t)bstride; a.theta = dd + nx + ny + nb; a.lml = dd + nin; a.rec = a.lml + R;
    a.n_begin = dnb;
    int* dlist = di + R;
    a.run_model = di; a.list = dlist; a.status = di + 2 * R; a.iters = di + 3 * R; a.evals = di + 4 * R; a.cnt = di + 5 * R;
    a.D = D; a.O = O; a.n_ls = n_ls; a.max_iter = max_iter; a.max_evals = max_evals; a.max_ls = BAT_OPT_MAX_LS;
    a.evals_per_launch = evals_per_launch; a.jitter = alpha_jitter; a.pgtol = pgtol; a.ftol = ftol;
    CALLCHK(hipMemcpyAsync(dd, hd.data(), nin * sizeof(double), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipMemcpyAsync(dnb, n_begin, ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipMemcpyAsync(di, run_model, (size_t)R * sizeof(int), hipMemcpyHostToDevice, buf.stream));
    CALLCHK(hipMemsetAsync(a.status, 0xFF, (size_t)R * sizeof(int), buf.stream));                 // BAT_OPT_LIVE
    CALLCHK(hipMemsetAsync(a.iters, 0, (size_t)R * (2 + BAT_OPT_CNT) * sizeof(int), buf.stream));   // iterations | evaluations | counters

    // every launch spends at least one evaluation of every live run, and a run ends at max_evals at the latest
    std::vector<int> st(R);
    for (int64_t round = 0; !live.empty(); ++round) {
        if (round > max_evals) return fail(GPT_E_HIP, w + ": runs still live after max_evals launches");
        CALLCHK(hipMemcpyAsync(dlist, live.data(), live.size() * sizeof(int), hipMemcpyHostToDevice, buf.stream));
        launch_bat_optimize(buf.stream, kernel_type, n_small, (int)live.size() - n_small, a);
        CALLCHK(hipGetLastError());
        CALLCHK(hipMemcpyAsync(st.data(), a.status, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, buf.stream));
        CALLCHK(hipStreamSynchronize(buf.stream));          // `live` is rewritten below
        size_t kept = 0;
        int kept_small = 0;
        for (size_t k = 0; k < live.size(); ++k)
            if (st[live[k]] == BAT_OPT_LIVE) {
                if ((int)k < n_small) ++kept_small;
                live[kept++] = live[k];
            }
        live.resize(kept);
        n_small = kept_small;
    }

    std::vector<double> out((size_t)R * (P + 1));            // theta | lml are adjacent on the device
    std::vector<int> outi((size_t)R * 2);                    // iterations | evaluations
    CALLCHK(hipMemcpyAsync(out.data(), a.theta, out.size() * sizeof(double), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipMemcpyAsync(outi.data(), a.iters, outi.size() * sizeof(int), hipMemcpyDeviceToHost, buf.stream));
    CALLCHK(hipStreamSynchronize(buf.stream));
    std::copy(out.begin(), out.begin() + (size_t)R * P, theta);
    std::copy(out.begin() + (size_t)R * P, out.end(), lml);
    std::copy(outi.begin(), outi.begin() + R, iterations);
    std::copy(outi.begin() + R, outi.end(), evaluations);
    std::copy(st.begin(), st.end(), status);
    return GPT_OK;
}

}  // namespace

extern "C" int gpt_batch_optimize(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O, int n_ls,
                                  const int* run_model, const double* theta0, int64_t R, const double* bounds, double alpha_jitter,
                                  int kernel_type, double pgtol, double ftol, int max_iter, int max_evals, int evals_per_launch,
                                  double* theta, double* lml, int* iterations, int* evaluations, int* status) {
    return batch_optimize("gpt_batch_optimize", false, device, X, Y, n_begin, B, D, O, n_ls, run_model, theta0, R, bounds, alpha_jitter,
                          kernel_type, pgtol, ftol, max_iter, max_evals, evals_per_launch, theta, lml, iterations, evaluations, status);
}

extern "C" int gpt_batch_optimize_bounded(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                                          int n_ls, const int* run_model, const double* theta0, int64_t R, const double* run_bounds,
                                          double alpha_jitter, int kernel_type, double pgtol, double ftol, int max_iter, int max_evals,
                                          int evals_per_launch, double* theta, double* lml, int* iterations, int* evaluations, int* status) {
    return batch_optimize("gpt_batch_optimize_bounded", true, device, X, Y, n_begin, B, D, O, n_ls, run_model, theta0, R, run_bounds,
                          alpha_jitter, kernel_type, pgtol, ftol, max_iter, max_evals, evals_per_launch, theta, lml, iterations, evaluations,
                          status);
}
