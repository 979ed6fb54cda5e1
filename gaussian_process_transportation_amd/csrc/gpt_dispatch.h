// Which kernel a launch takes, decided in one place each (device units only): a run-time value becomes a compile-time one
// and is handed to a generic lambda, which names the instantiation; and the launch that may use dynamic LDS beyond the default.
#pragma once
#include "gpt_common.h"
#include "gpt_exp.h"
#include <type_traits>

namespace gpt {

// Launches Kernel with `lds` bytes of dynamic LDS.  More than the default limit is an opt-in per kernel and device; it is made
// here, before the first launch on each device, so a kernel that is launched has it.  (`lds` is a constant of the kernel.)
template <auto Kernel, class... A>
void launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, A... a) {
    static PerDeviceOnce once;
    once.run([&] { hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, a...);
}

template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;

// f(Int<DW>{}), DW = coord_width(D): the DW template argument of the kernels that carry coordinates
template <class F> void with_coord_width(int D, F&& f) {
    if (D <= 3) f(Int<3>{});
    else if (D <= WIDE_D) f(Int<WIDE_D>{});
    else f(Int<MAX_D>{});
}
// f(T{}), T = the element type `dtype` (DT_F64 / DT_F32) names
template <class F> void with_elem_type(int dtype, F&& f) {
    if (dtype == DT_F32) f(float{});
    else f(double{});
}
// f(Int<KT>{}), KT = ktype (gpt_exp.h; anything else: RBF)
template <class F> void with_kernel_type(int ktype, F&& f) {
    switch (ktype) {
        case KT_MATERN12: f(Int<KT_MATERN12>{}); break;
        case KT_MATERN32: f(Int<KT_MATERN32>{}); break;
        case KT_MATERN52: f(Int<KT_MATERN52>{}); break;
        default: f(Int<KT_RBF>{});
    }
}

}  // namespace gpt
