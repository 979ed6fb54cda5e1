// Launchers of the residue (int8) variance path: the image of W in residue planes (once per model) and the k*-alone variance of
// an fp64 single-task model, D <= 3.  Kernels: gpt_kvar_i8.h; arithmetic and plan: gpt_plan_i8.h; who takes the path: gpt_api.hip.
#include "gpt_common.h"
#include "gpt_kvar_i8.h"
#include <cstdlib>

namespace gpt {

void launch_var_i8_image(hipStream_t s, const double* Wf, int NP, int bits, void* planes, double* rowscale, double* qscale, void* rowmax) {
    const int nbi = NP / I8_ROWS, ntiles = nbi * (nbi + 1) / 2;
    unsigned long long* rm = static_cast<unsigned long long*>(rowmax);
    (void)hipMemsetAsync(rm, 0, (size_t)NP * sizeof(unsigned long long), s);
    const dim3 grid(ntiles, 8);
    hipLaunchKernelGGL(k_i8_rowmax, grid, dim3(256), 0, s, Wf, rm);
    hipLaunchKernelGGL(k_i8_rowscale, dim3((NP + 255) / 256), dim3(256), 0, s, rm, NP, bits, rowscale, qscale);
    hipLaunchKernelGGL(k_i8_planes, grid, dim3(256), 0, s, Wf, qscale, ntiles, static_cast<v4i*>(planes));
}

void launch_var_i8(hipStream_t s, const KernelParams& p, const VarI8PlanDev& plan, int bits, const void* planes, const double* rowscale,
                   const double* Xs, const double* Xq, int64_t M, double* slab, void* bimg, void* park, double* var, const double* hdr) {
    if (M <= 0) return;
    VarI8Args a{};
    a.planes = static_cast<const v4i*>(planes); a.rowscale = rowscale; a.Xs = Xs; a.Xq = Xq; a.M = M;
    a.slab = slab; a.bimg = static_cast<v4i*>(bimg); a.park = static_cast<unsigned*>(park);
    const int f = var_i8_exponent(p.c);                  // one column exponent, from the prior variance: k* <= c <= 2^f
    a.bq = std::ldexp(1.0, bits - f);
    a.colscale = std::ldexp(1.0, f - bits);
    a.ntiles = plan.nbi * (plan.nbi + 1) / 2;
    // rounds per launch (var_i8_rounds_per_launch): workgroups that drift apart stop sharing the A stream in L2, and a kernel boundary
    // brings them together.  One round, measured on this kernel at N = 8192, M = 500 000 (profiles/var_int8_feed.txt: var_ms 277.2 /
    // 280.8 / 285.6 / 287.6 / 289.2 for 1 / 2 / 3 / 4 / 16 = all in one launch; launch_var's 16 had been inherited unmeasured)
    const int64_t rounds = plan.nfull / plan.P;
    const int64_t rpl = var_i8_rounds_per_launch(plan);
    const int npairs = var_i8_npairs(plan.nbi), spl = var_i8_item_steps_per_launch(plan);
    // a group's images (k_i8_gen), then the sweeps of its items; the tail's blocks are a group of their own
    auto group = [&](int64_t r0, int64_t r1, int64_t nimg, bool tail) {
        VarI8PlanDev pl = plan;
        pl.rnd_begin = r0; pl.rnd_end = r1; pl.with_tail = tail ? 1 : 0;
        with_kernel_type(p.ktype, [&](auto kt) {
            constexpr int KT = decltype(kt)::value;
            if (!I8_ABL_NOGEN)
                hipLaunchKernelGGL(k_i8_gen<KT>, dim3((unsigned)nimg, (unsigned)plan.nbi), dim3(512), 0, s, p, a, r0 * plan.P);
            for (int k0 = 0; k0 == 0 || (!tail && k0 < npairs); k0 += spl) {
                pl.step_begin = tail ? 0 : k0;
                pl.step_end = tail ? 0 : (k0 + spl < npairs ? k0 + spl : npairs);
                launch_lds<k_var_i8<KT>>(dim3((unsigned)plan.P), dim3(512), I8_LDS_BYTES, s, p, pl, a);
            }
        });
    };
    for (int64_t r0 = 0; r0 < rounds; r0 += rpl) {
        const int64_t r1 = r0 + rpl < rounds ? r0 + rpl : rounds;
        group(r0, r1, (r1 - r0) * plan.P, false);
    }
    if (plan.ncb > plan.nfull) group(rounds, rounds, plan.ncb - plan.nfull, true);
    hipLaunchKernelGGL(k_var_i8_finalize, dim3((unsigned)plan.ncb), dim3(I8_COLS), 0, s, p, plan.nbi, slab, M, hdr, var);
}

}  // namespace gpt
