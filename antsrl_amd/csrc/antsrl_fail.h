// antsrl_fail.h — how every C-ABI entry of the library reports an error, whichever translation unit holds it: the
// message goes to the calling thread's antsrl_last_error(), the code is returned.  Defined in antsrl_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

#define ANTSRL_INTERNAL __attribute__((visibility("hidden")))

ANTSRL_INTERNAL int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
ANTSRL_INTERNAL int hip_fail(hipError_t e, const char *what); // ANTSRL_E_DEVICE, "<what>: <hipGetErrorString(e)>"
