// The host side that the .hip translation units of libmeerqat_hip.so share: ONE way for a failing HIP call to become MQ_EHIP with
// the error recorded for mq_last_hip_error(), and the dynamic-LDS attribute of a kernel raised once per device.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

#include "../../include/meerqat_hip.h"

extern "C" void mq_internal_set_hip_error(int e);  // knn.hip: the calling thread's mq_last_hip_error()

// in a function that returns an MQ_* status: on failure record the error and return MQ_EHIP
#define MQ_HIP(call)                               \
    do {                                           \
        hipError_t _e = (call);                    \
        if (_e != hipSuccess) {                    \
            mq_internal_set_hip_error((int)_e);    \
            return MQ_EHIP;                        \
        }                                          \
    } while (0)

// the status of the kernel launch(es) just made
inline int mq_launch_status() {
    MQ_HIP(hipGetLastError());
    return MQ_OK;
}

namespace mq_detail {

constexpr int LDS_PER_CU = 160 * 1024;  // gfx950

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): raise it the first time a
// kernel is launched on a device instead of on every call.  `done` = one bit per device ordinal.
inline hipError_t ensure_dynamic_lds(const void* fn, int bytes, std::atomic<unsigned long long>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    if (bytes >= LDS_PER_CU) {  // "as much as the kernel may ever ask for": what its static __shared__ objects leave
        hipFuncAttributes attr;
        e = hipFuncGetAttributes(&attr, fn);
        if (e != hipSuccess) return e;
        bytes = LDS_PER_CU - (int)attr.sharedSizeBytes;
    }
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

}  // namespace mq_detail

// the kernel expression may hold commas
#define MQ_DYNAMIC_LDS(bytes, ...)                                                                      \
    do {                                                                                               \
        static std::atomic<unsigned long long> _mq_lds_done{0};                                        \
        MQ_HIP(mq_detail::ensure_dynamic_lds((const void*)(__VA_ARGS__), (int)(bytes), _mq_lds_done)); \
    } while (0)
