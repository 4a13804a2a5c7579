// antsrl_memagent_dev.h — the device helpers of the agents' loop kernels that a population runs too: the action part of
// k_agent_select (antsrl_agent_select_actions.inc) and the whole of k_replay_record (antsrl_replay_record_body.inc) are
// texts included inside those kernels (antsrl_memagent.hip) and inside k_pop_select and k_pop_record
// (antsrl_population.hip); what the texts call is here.  The draw specification is written out in include/antsrl.h;
// the device functions of antsrl_draw.h are that text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_draw.h"
#include "antsrl_memagent.h"
#include "antsrl_util.h"

// ------------------------------------------------------------------ antsrl_agent_select
__device__ __forceinline__ bool env_explores(const SelArgs &a, uint32_t e)
{
    return draw_u01(agent_draw(a.seed, ANTSRL_DRAW_EXPLORE, (uint64_t)a.env_base + e, a.step, 0)) < a.epsilon;
}

// ------------------------------------------------------------------ antsrl_replay_record_pre / _post
// 4 consecutive elements at p as floats.  mode 0: one load of the 4 (16 bytes float32, 8 bytes bfloat16), 1: two loads,
// 2: four.  The caller picks the mode from p's alignment.
template <bool BF16>
__device__ __forceinline__ float4 load4(const void *p, int mode)
{
    if (BF16) {
        uint32_t lo, hi;
        if (mode == 0) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p);
            lo = v.x; hi = v.y;
        } else if (mode == 1) {
            lo = reinterpret_cast<const uint32_t *>(p)[0];
            hi = reinterpret_cast<const uint32_t *>(p)[1];
        } else {
            const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
            lo = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
            hi = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
        }
        return make_float4(__uint_as_float(lo << 16), __uint_as_float(lo & 0xFFFF0000u), __uint_as_float(hi << 16),
                           __uint_as_float(hi & 0xFFFF0000u));
    }
    if (mode == 0) return *reinterpret_cast<const float4 *>(p);
    if (mode == 1) {
        const float2 l = reinterpret_cast<const float2 *>(p)[0], h = reinterpret_cast<const float2 *>(p)[1];
        return make_float4(l.x, l.y, h.x, h.y);
    }
    const float *q = reinterpret_cast<const float *>(p);
    return make_float4(q[0], q[1], q[2], q[3]);
}

template <bool BF16>
__device__ __forceinline__ float load1(const void *base, int i)
{
    if (BF16) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(base)[i] << 16);
    return reinterpret_cast<const float *>(base)[i];
}
