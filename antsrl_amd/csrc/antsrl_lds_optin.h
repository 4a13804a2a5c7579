// antsrl_lds_optin.h — host helper: more than 64 KiB of dynamic LDS is an opt-in per kernel function and per device.
#pragma once
#include <hip/hip_runtime.h>

#define ANTSRL_MAX_DEVICES 64 // per-device launch bookkeeping

// Raises Kernel's dynamic-LDS limit on the current device to `bytes` if that is more than it has been given there (a grant
// is recorded only when it succeeded).  The table is per kernel and per translation unit: launch a kernel from one unit.
template <auto Kernel>
static inline hipError_t antsrl_lds_optin(size_t bytes)
{
    static size_t given[ANTSRL_MAX_DEVICES] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= ANTSRL_MAX_DEVICES) return hipErrorInvalidDevice;
    if (bytes <= given[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) given[dev] = bytes;
    return e;
}
