// antsrl_fail.h — how every C-ABI entry of the library reports an error, whichever translation unit holds it: the
// message goes to the calling thread's antsrl_last_error(), the code is returned.  Defined in antsrl_capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/antsrl.h"

#define ANTSRL_INTERNAL __attribute__((visibility("hidden")))

ANTSRL_INTERNAL int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
ANTSRL_INTERNAL int hip_fail(hipError_t e, const char *what); // ANTSRL_E_DEVICE, "<what>: <hipGetErrorString(e)>"

// what an entry returns behind its last launch or copy
static inline int enqueued(hipError_t e, const char *who) { return e != hipSuccess ? hip_fail(e, who) : ANTSRL_OK; }

// a pointer argument of an entry (`who` in scope), named in the message as the ABI names it: not NULL, aligned
#define REQUIRE(p, align)                                                                                                \
    do {                                                                                                                 \
        if (!(p)) return fail(ANTSRL_E_INVALID, "%s: %s is required", who, #p);                                          \
        if ((uintptr_t)(p) & ((align) - 1)) return fail(ANTSRL_E_INVALID, "%s: %s must be %d-byte aligned", who, #p, (int)(align)); \
    } while (0)

// REQUIRE for a pointer that the entries of a shared body name differently: `name` is the ABI's
static inline int require_named(const char *who, const char *name, const void *p, int align)
{
    if (!p) return fail(ANTSRL_E_INVALID, "%s: %s is required", who, name);
    if ((uintptr_t)p & (uintptr_t)(align - 1)) return fail(ANTSRL_E_INVALID, "%s: %s must be %d-byte aligned", who, name, align);
    return ANTSRL_OK;
}
