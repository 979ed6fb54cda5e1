// Host helpers of the C entry points (internal header; plain C++, it also compiles under g++ against host_stub/, the sanitizer
// builds).  fail() and CALLCHK serve every unit, gpt_api.hip included.  The rest is for a one-shot call without a handle, which
// validates host arrays, opens a stream, allocates, enqueues its whole schedule through its unit's launchers, reads back and
// frees: gpt_svgp_train_host.hip, gpt_svgp_surface_host.hip, gpt_select_host.hip, gpt_batch_host.hip, gpt_batch_opt_host.hip, gpt_fold_scan_host.hip (all six run under the
// sanitizers: make host-oneshot-asan) and gpt_debug_dgemm (gpt_fit.hip).  gpt_transport_host.hip and gpt_chain_host.hip have the
// same layout but work on handles, which keep what they allocate; what those two and gpt_api.hip share is in gpt_stage.h.  A
// handle's long-lived resources have owners of their own: DevBuf, Stream and Event in gpt_common.h.
#pragma once
#include "gpt_common.h"
#include "../../include/gpt_hip.h"

#include <climits>
#include <cmath>
#include <string>
#include <vector>

namespace gpt {

// Sets the calling thread's gpt_last_error() text; returns the code.
inline int fail(int code, const std::string& msg) {
    set_last_error(msg.c_str());
    return code;
}

// Returns GPT_E_HIP from the enclosing function if a hipError_t expression fails.
#define CALLCHK(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return gpt::fail(GPT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Stream and device buffers of one call; synchronised and released on every return path.
struct CallBuffers {
    std::vector<void*> ptrs;
    hipStream_t stream = nullptr;
    ~CallBuffers() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (void* p : ptrs) (void)hipFree(p);
    }
    hipError_t open() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
    template <class T> hipError_t alloc(T** p, size_t count) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 8);
        if (e == hipSuccess) ptrs.push_back(q);
        *p = static_cast<T*>(q);
        return e;
    }
};

inline bool all_finite(const double* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// Makes `device` the calling thread's device; GPT_E_ARG if there is no such device.
inline int use_device(const std::string& who, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(GPT_E_ARG, who + ": no such HIP device");
    CALLCHK(hipSetDevice(device));
    return GPT_OK;
}

}  // namespace gpt
