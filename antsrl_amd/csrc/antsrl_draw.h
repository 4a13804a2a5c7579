// antsrl_draw.h — the draw specification of include/antsrl.h ("THE DRAW SPECIFICATION") as device functions, for the
// kernels that draw from it: antsrl_memagent.hip (select, plan, record) and antsrl_rework.hip (act + select).
//     agent_draw(seed, tag, env, step, item) = draw_item(draw_env_step(seed, env, step), item, tag)
// The first two rounds of a draw depend on the environment and the step alone: a kernel that makes several draws for one
// environment keeps draw_env_step's key and pays two rounds per draw.
#pragma once
#include <stdint.h>
#include "antsrl_util.h"

__device__ __forceinline__ uint64_t draw_env_step(uint64_t seed, uint64_t env, uint64_t step)
{
    const uint64_t k = mix64(seed + 0x9E3779B97F4A7C15ULL * (env + 1));
    return mix64(k ^ (0xD1B54A32D192ED03ULL * (step + 1)));
}
__device__ __forceinline__ uint64_t draw_item(uint64_t env_step_key, uint64_t item, uint64_t tag)
{
    return mix64(mix64(env_step_key + 0x9E3779B97F4A7C15ULL * (item + 1)) ^ tag);
}
__device__ __forceinline__ uint64_t agent_draw(uint64_t seed, uint64_t tag, uint64_t env, uint64_t step, uint64_t item)
{
    return draw_item(draw_env_step(seed, env, step), item, tag);
}
__device__ __forceinline__ double draw_u01(uint64_t k) { return (double)(k >> 11) * (1.0 / 9007199254740992.0); }
__device__ __forceinline__ uint32_t draw_below(uint64_t k, uint32_t n) { return (uint32_t)(((k >> 32) * (uint64_t)n) >> 32); }
