// gpt_select_greedy (include/gpt_hip.h): argument checks, the memory estimate, the buffers of one call, the uploads and the
// read-back.  Host code only (the kernels: gpt_select.hip, reached through the launcher of gpt_select.h), so it also compiles
// under g++ against host_stub/ and runs under the sanitizers (make host-oneshot-asan).
#include "gpt_select.h"
#include "gpt_call.h"

namespace {
constexpr double SEL_MEMORY_SHARE = 0.8; // of the device's free memory the pool factor may take
}

using namespace gpt;

extern "C" int gpt_select_greedy(int device, const double* X, int64_t N, int D, const double* length_scale, double c, double noise,
                                 double alpha, int kernel_type, const int64_t* initial, int n_initial, int n_total, int64_t* selected,
                                 double* selection_variance, double* residual_variance) {
    const std::string w = "gpt_select_greedy";
    if (!X || !length_scale || !selected || (n_initial > 0 && !initial) || (n_total > n_initial && !selection_variance))
        return fail(GPT_E_ARG, w + ": NULL argument");
    if (D < 1 || D > MAX_DIMS) return fail(GPT_E_ARG, w + ": D must be 1 .. 15, got " + std::to_string(D));
    if (N < 1 || N > INT_MAX) return fail(GPT_E_ARG, w + ": N must be 1 .. 2^31 - 1");
    if (n_total < 1 || n_initial < 0 || n_initial > n_total)
        return fail(GPT_E_ARG, w + ": need 0 <= n_initial <= n_total and n_total >= 1");
    if (n_total > N)
        return fail(GPT_E_ARG, w + ": cannot select " + std::to_string(n_total) + " points from a pool of " + std::to_string(N));
    if (kernel_type < GPT_KERNEL_RBF || kernel_type > GPT_KERNEL_MATERN52) return fail(GPT_E_ARG, w + ": unknown kernel_type");
    if (!(c > 0) || !std::isfinite(c) || !(noise >= 0) || !std::isfinite(noise) || !(alpha >= 0) || !std::isfinite(alpha))
        return fail(GPT_E_ARG, w + ": need finite constant_value > 0, noise >= 0, alpha >= 0");
    double inv_ls[MAX_D] = {};
    for (int k = 0; k < D; ++k) {
        if (!(length_scale[k] > 0) || !std::isfinite(length_scale[k])) return fail(GPT_E_ARG, w + ": length_scale must be finite and > 0");
        inv_ls[k] = 1.0 / length_scale[k];
    }
    // sizes first: a pool that cannot fit is refused before it is read
    if (int rc = use_device(w, device)) return rc;

    const int mp = n_total + (n_total & 1);        // rows of P stay 16-byte aligned
    const int stride = xs_stride(D);
    size_t mem_free = 0, mem_total = 0;
    CALLCHK(hipMemGetInfo(&mem_free, &mem_total));
    // everything the call allocates that grows with N: the pool factor, the raw and the scaled pool, d, the alive mask
    const double factor = 8.0 * (double)N * mp;
    const double need = factor + (double)N * (8.0 * D + 8.0 * stride + 8.0 + 1.0) + 16.0 * n_total + 65536.0;
    if (need > SEL_MEMORY_SHARE * (double)mem_free)
        return fail(GPT_E_ARG, w + ": the call needs " + std::to_string((long long)(need / 1048576.0)) + " MiB of device memory (pool factor 8 N m = " +
                                       std::to_string((long long)(factor / 1048576.0)) + " MiB), more than " +
                                       std::to_string((int)(SEL_MEMORY_SHARE * 100)) + " % of the device's free memory (" +
                                       std::to_string((long long)(mem_free / 1048576)) + " MiB free)");

    // without an initial subset every point starts at the prior variance and the lowest index wins: pivot 0
    const int n_pre = n_initial > 0 ? n_initial : 1;
    std::vector<int> sel32(n_total, 0);
    {
        std::vector<unsigned char> seen(N, 0);
        for (int t = 0; t < n_initial; ++t) {
            if (initial[t] < 0 || initial[t] >= N) return fail(GPT_E_ARG, w + ": initial index out of range at " + std::to_string(t));
            if (seen[initial[t]]) return fail(GPT_E_ARG, w + ": initial index " + std::to_string(initial[t]) + " is listed twice");
            seen[initial[t]] = 1;
            sel32[t] = (int)initial[t];
        }
    }
    for (size_t e = 0; e < (size_t)N * D; ++e)
        if (!std::isfinite(X[e])) return fail(GPT_E_ARG, w + ": the pool contains NaN or infinity (row " + std::to_string(e / D) + ")");
    CallBuffers buf;
    CALLCHK(buf.open());
    const hipStream_t s = buf.stream;
    SelArgs a{};
    double *dX, *dXs, *dP, *dd, *dpivd, *dpart_d, *dinv;
    unsigned char* dalive;
    int *dsel, *dpart_i, *dfail;
    CALLCHK(buf.alloc(&dX, (size_t)N * D));
    CALLCHK(buf.alloc(&dinv, (size_t)MAX_D));
    CALLCHK(buf.alloc(&dXs, (size_t)N * stride));
    CALLCHK(buf.alloc(&dP, (size_t)N * mp));
    CALLCHK(buf.alloc(&dd, (size_t)N));
    CALLCHK(buf.alloc(&dalive, (size_t)N));
    CALLCHK(buf.alloc(&dsel, (size_t)n_total));
    CALLCHK(buf.alloc(&dpivd, (size_t)n_total));
    CALLCHK(buf.alloc(&dpart_d, (size_t)SEL_MAX_WG));
    CALLCHK(buf.alloc(&dpart_i, (size_t)SEL_MAX_WG));
    CALLCHK(buf.alloc(&dfail, 1));
    CALLCHK(hipMemcpyAsync(dX, X, (size_t)N * D * 8, hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(dinv, inv_ls, sizeof(inv_ls), hipMemcpyHostToDevice, s));
    CALLCHK(hipMemcpyAsync(dsel, sel32.data(), (size_t)n_total * sizeof(int), hipMemcpyHostToDevice, s));
    CALLCHK(hipMemsetAsync(dP, 0, (size_t)N * mp * 8, s));
    CALLCHK(hipMemsetAsync(dfail, 0, sizeof(int), s));
    a.Xs = dXs; a.P = dP; a.d = dd; a.alive = dalive; a.selected = dsel; a.pivd = dpivd; a.part_d = dpart_d; a.part_i = dpart_i;
    a.fail = dfail; a.N = (int)N; a.stride = stride; a.mp = mp; a.n_pre = n_pre; a.ktype = kernel_type;
    a.lnc = std::log(c); a.base_var = c + noise; a.alpha = alpha;

    launch_sel_schedule(s, a, dX, dinv, dXs, D, n_total);
    CALLCHK(hipGetLastError());
    int failed = 0;
    std::vector<double> pivd(n_total);
    CALLCHK(hipMemcpyAsync(&failed, dfail, sizeof(int), hipMemcpyDeviceToHost, s));
    CALLCHK(hipMemcpyAsync(sel32.data(), dsel, (size_t)n_total * sizeof(int), hipMemcpyDeviceToHost, s));
    CALLCHK(hipMemcpyAsync(pivd.data(), dpivd, (size_t)n_total * 8, hipMemcpyDeviceToHost, s));
    CALLCHK(hipStreamSynchronize(s));
    if (failed)
        return fail(GPT_E_NOT_PD, w + ": non-positive pivot (residual variance + alpha <= 0) at insertion " + std::to_string(failed - 1) +
                                          ": the selected points' kernel matrix is not positive definite");
    if (residual_variance) {
        CALLCHK(hipMemcpyAsync(residual_variance, dd, (size_t)N * 8, hipMemcpyDeviceToHost, s));
        CALLCHK(hipStreamSynchronize(s));
    }
    for (int t = 0; t < n_total; ++t) selected[t] = sel32[t];
    for (int t = n_initial; t < n_total; ++t) selection_variance[t - n_initial] = pivd[t];
    return GPT_OK;
}
