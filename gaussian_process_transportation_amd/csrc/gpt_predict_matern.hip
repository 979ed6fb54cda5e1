// k_var launches with derivative columns (Jacobian variance, d var) of Matern 3/2 and 5/2 models, in a translation unit of their
// own, compiled beside gpt_predict.hip (which keeps every other instantiation) by a parallel build.  The kernel is gpt_kvar.h's k_var with KT =
// KT_MATERN32 / KT_MATERN52: a derivative column takes c g(r) u_d instead of c k(r) u_d (gpt_exp.h), the reload sweeps are the
// same code.  No HALF instantiations: the plain kernel runs at every model size ("Matern derivatives").
#include "gpt_kvar.h"

namespace gpt {

template <typename T, int KT>
static void var_kernel_setup_matern() {
    static PerDeviceOnce once;
    once.run([] {
        const void* fns[] = {reinterpret_cast<const void*>(k_var<T, 4, true, KT>), reinterpret_cast<const void*>(k_var<T, 4, false, KT>),
                             reinterpret_cast<const void*>(k_var<T, 3, false, KT>),
                             reinterpret_cast<const void*>(k_var<T, 8, true, KT, WIDE_D>), reinterpret_cast<const void*>(k_var<T, 8, false, KT, WIDE_D>),
                             reinterpret_cast<const void*>(k_var<T, 16, true, KT, WIDE_D>), reinterpret_cast<const void*>(k_var<T, 16, false, KT, WIDE_D>),
                             reinterpret_cast<const void*>(k_var<T, 4, false, KT, WIDE_D, false>), reinterpret_cast<const void*>(k_var<T, 8, false, KT, WIDE_D, false>),
                             reinterpret_cast<const void*>(k_var<T, 16, true, KT, MAX_D>), reinterpret_cast<const void*>(k_var<T, 16, false, KT, MAX_D>)};
        for (const void* f : fns) hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)var_lds_bytes<T>());
    });
}

// the same ncomp / D cases as launch_var_t in gpt_predict.hip
template <typename T, int KT>
static void launch_var_kt(hipStream_t s, const KernelParams& p, const VarPlanDev& pl, int ncomp, bool cross, dim3 grid, size_t lds,
                          const T* Xs, const T* Wf, const T* Xq, int64_t M, T* slab, T* vslab, T* bscr) {
    var_kernel_setup_matern<T, KT>();
#define GPT_KVARM(NC_, CR_, DW_, KS_) hipLaunchKernelGGL((k_var<T, NC_, CR_, KT, DW_, KS_>), grid, dim3(512), lds, s, p, pl, Xs, Wf, Xq, M, slab, vslab, bscr)
    const bool wide16 = p.D > WIDE_D;
    if (ncomp == VAR_NCOMP_DERIV4) GPT_KVARM(4, false, WIDE_D, false);           // D = 4, Jacobian variance alone
    else if (ncomp == VAR_NCOMP_DERIV8) GPT_KVARM(8, false, WIDE_D, false);      // D = 8
    else if (ncomp == 3) GPT_KVARM(3, false, 3, true);                           // D <= 3, Jacobian variance alone
    else if (ncomp == 4) { if (cross) GPT_KVARM(4, true, 3, true); else GPT_KVARM(4, false, 3, true); }
    else if (ncomp == 8) { if (cross) GPT_KVARM(8, true, WIDE_D, true); else GPT_KVARM(8, false, WIDE_D, true); }     // D = 4 .. 7
    else if (wide16) { if (cross) GPT_KVARM(16, true, MAX_D, true); else GPT_KVARM(16, false, MAX_D, true); }        // D = 9 .. 15
    else { if (cross) GPT_KVARM(16, true, WIDE_D, true); else GPT_KVARM(16, false, WIDE_D, true); }                   // D = 8
#undef GPT_KVARM
}

template <typename T>
void launch_var_matern(hipStream_t s, const KernelParams& p, const VarPlanDev& pl, int ncomp, bool cross, dim3 grid, size_t lds,
                       const T* Xs, const T* Wf, const T* Xq, int64_t M, T* slab, T* vslab, T* bscr) {
    if (p.ktype == KT_MATERN32) launch_var_kt<T, KT_MATERN32>(s, p, pl, ncomp, cross, grid, lds, Xs, Wf, Xq, M, slab, vslab, bscr);
    else launch_var_kt<T, KT_MATERN52>(s, p, pl, ncomp, cross, grid, lds, Xs, Wf, Xq, M, slab, vslab, bscr);
}

template void launch_var_matern<double>(hipStream_t, const KernelParams&, const VarPlanDev&, int, bool, dim3, size_t, const double*,
                                        const double*, const double*, int64_t, double*, double*, double*);
template void launch_var_matern<float>(hipStream_t, const KernelParams&, const VarPlanDev&, int, bool, dim3, size_t, const float*,
                                       const float*, const float*, int64_t, float*, float*, float*);

}  // namespace gpt
