// k_var launches with derivative columns (Jacobian variance, d var) of Matern 3/2 and 5/2 models, in a translation unit of their
// own, compiled beside gpt_predict.hip (which keeps every other instantiation) by a parallel build.  The kernel is gpt_kvar.h's k_var with KT =
// KT_MATERN32 / KT_MATERN52: a derivative column takes c g(r) u_d instead of c k(r) u_d (gpt_exp.h), the reload sweeps are the
// same code.  No HALF instantiations: the plain kernel runs at every model size ("Matern derivatives").
#include "gpt_kvar.h"

namespace gpt {

template <typename T>
void launch_var_matern(hipStream_t s, const KernelParams& p, const VarPlanDev& pl, int ncomp, bool cross, dim3 grid,
                       const T* Xs, const T* Wf, const T* Xq, int64_t M, T* slab, T* vslab, T* bscr) {
    if (p.ktype == KT_MATERN32) launch_kvar<T, KT_MATERN32, true>(ncomp, cross, p.D, false, grid, s, p, pl, Xs, Wf, Xq, M, slab, vslab, bscr);
    else launch_kvar<T, KT_MATERN52, true>(ncomp, cross, p.D, false, grid, s, p, pl, Xs, Wf, Xq, M, slab, vslab, bscr);
}

template void launch_var_matern<double>(hipStream_t, const KernelParams&, const VarPlanDev&, int, bool, dim3, const double*,
                                        const double*, const double*, int64_t, double*, double*, double*);
template void launch_var_matern<float>(hipStream_t, const KernelParams&, const VarPlanDev&, int, bool, dim3, const float*,
                                       const float*, const float*, int64_t, float*, float*, float*);

}  // namespace gpt
