// antsrl_memagent.h — arguments and launchers of the agents' loop's kernels (antsrl_memagent.hip), shared with their
// C-ABI entries (antsrl_loopapi.hip; the entries' argument rules: antsrl_loopapi.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_fail.h"

struct SelArgs {
    uint64_t seed, step;
    double epsilon;
    int8_t *rot, *ph;
    const float *mem_old;
    float *mem_next;
    uint8_t *explored;
    uint32_t env_base, n_ants, n_rot, n_ph;
    uint32_t M;         // ants
    uint32_t env_elems; // memory elements (floats, or float4 when V == 4) per environment
    uint64_t mem_elems; // memory elements of the batch
};

struct RecArgs {
    const void *obs;
    const float *agent_state, *memory, *reward;
    const int8_t *rot, *ph;
    const uint8_t *done;
    float *states, *agent_states, *rewards; // (new_states / new_agent_states in the post half)
    int64_t *actions;
    uint8_t *dones;
    uint64_t seed, step, env_base;
    long long M, K;
    long long j0, n_write; // entries j0 .. j0 + n_write - 1 are written (n_write <= max_len)
    long long row0, max_len; // ring row of entry j0
    long long pitch;       // elements between two ants' observation rows
    int n_ants, F, A, mem, half_rot;
};

// vec: the memory copy moves float4 elements (env_elems / mem_elems count those); post: the half behind the environment step
ANTSRL_INTERNAL hipError_t antsrl_launch_agent_select(const SelArgs &a, bool vec, hipStream_t st);
// the plan reads seed, step, epsilon, env_base, n_ants and M of `a` (select's own arguments: one env_explores for both)
ANTSRL_INTERNAL hipError_t antsrl_launch_agent_plan(const SelArgs &a, int32_t *tiles, int32_t *n_live, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_replay_record(const RecArgs &a, bool obs_bf16, bool post, hipStream_t st);
