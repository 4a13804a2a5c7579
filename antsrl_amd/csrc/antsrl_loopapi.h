// antsrl_loopapi.h — the argument rules of the agents' loop (antsrl_loopapi.hip), for every API file that has one of
// them: the single agents' entries, the population's (antsrl_popapi.hip: the same rule per member) and the rework
// agent's fused act + select (antsrl_reworkapi.hip).  Host-side only; every function returns ANTSRL_OK or the refusal
// (message set, `who` the entry's name) and makes no HIP call.
#pragma once
#include <stdint.h>
#include "antsrl_fail.h"
#include "antsrl_memagent.h" // SelArgs, RecArgs

// n_envs, n_ants >= 1, n_envs * n_ants < 2^31, env_id_base >= 0, env_id_base + n_envs < 2^31
ANTSRL_INTERNAL int antsrl_check_batch(const char *who, int32_t env_id_base, int32_t n_envs, int32_t n_ants);
// the shape limits of the memory net's kernels, which a record's spec shares with the net's entries (antsrl_memapi.hip):
// a width (agent_dim, mem_size, n_rot, n_ph) <= 32, D = n_features + agent_dim + mem_size <= 1024
ANTSRL_INTERNAL int antsrl_check_max32(const char *who, const char *name, int32_t v);
ANTSRL_INTERNAL int antsrl_check_D(const char *who, int32_t n_features, int32_t agent_dim, int32_t mem_size);
// epsilon in [0, 1] (a NaN is refused); member >= 0: the message names that member of a population
ANTSRL_INTERNAL int antsrl_check_epsilon(const char *who, int member, double epsilon);
// ANTSRL_OBS_F32 or ANTSRL_OBS_BF16
ANTSRL_INTERNAL int antsrl_check_obs_format(const char *who, int obs_format);

// *a = the select (or plan) kernel's arguments of a batch its entry has checked: every pointer NULL and no memory part
ANTSRL_INTERNAL void antsrl_sel_args(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants,
                                     double epsilon, int32_t n_rot, int32_t n_ph, SelArgs *a);

// The ring rule: K of a step's `rows` transitions (`rows_words` says in the entry's own terms what `rows` is) go to
// the rows behind `head` of a ring of max_len.  Checks K, max_len and head and fills K, n_write, j0, row0 and max_len.
ANTSRL_INTERNAL int antsrl_ring_rows(const char *who, const char *rows_words, long long rows, int64_t K, int64_t head,
                                     int64_t max_len, RecArgs *a);

// The two halves of a record entry, for an *a that holds the entry's spec (a->mem: memory is required exactly when it is
// > 0): the half's pointers, required and aligned under the names include/antsrl.h gives them, into *a.
ANTSRL_INTERNAL int antsrl_rec_pre(const char *who, RecArgs *a, bool obs_bf16, const void *obs, const float *agent_state,
                                   const float *memory, const int8_t *rotation, const int8_t *pheromone, float *states,
                                   float *agent_states, int64_t *actions);
ANTSRL_INTERNAL int antsrl_rec_post(const char *who, RecArgs *a, bool obs_bf16, const void *obs, const float *agent_state,
                                    const float *memory, const float *reward, const uint8_t *done, float *rewards,
                                    float *new_states, float *new_agent_states, uint8_t *dones);
