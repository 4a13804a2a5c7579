// antsrl_loopapi.hip — the agents' loop in the C-ABI of libantsrl_hip.so (include/antsrl.h): antsrl_agent_select,
// antsrl_agent_plan and antsrl_replay_record_pre / _post for an agent with a memory, antsrl_agent_select_actions and
// antsrl_replay_record_pre_plain / _post_plain for one without (the same kernels without a memory operand), and the
// argument rules they share with the population's entries and the rework agent's fused act + select (antsrl_loopapi.h).
//
// Host-side only: validates the arguments and enqueues the kernels of antsrl_memagent.hip on the caller's stream.  No
// handle, no allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_device.h"
#include "antsrl_fail.h"
#include "antsrl_loopapi.h"
#include "antsrl_memagent.h"

// ---- the rules (antsrl_loopapi.h)
int antsrl_check_batch(const char *who, int32_t env_id_base, int32_t n_envs, int32_t n_ants)
{
    if (n_envs < 1 || n_ants < 1) return fail(ANTSRL_E_INVALID, "%s: n_envs and n_ants must be >= 1 (%d, %d)", who, n_envs, n_ants);
    if ((long long)n_envs * n_ants > 0x7fffffffLL)
        return fail(ANTSRL_E_INVALID, "%s: n_envs * n_ants = %lld must stay below 2^31", who, (long long)n_envs * n_ants);
    if (env_id_base < 0 || (long long)env_id_base + n_envs > 0x7fffffffLL)
        return fail(ANTSRL_E_INVALID, "%s: env_id_base must be >= 0 and env_id_base + n_envs must fit 31 bits", who);
    return ANTSRL_OK;
}

int antsrl_check_max32(const char *who, const char *name, int32_t v)
{
    if (v > 32) return fail(ANTSRL_E_UNSUPPORTED, "%s: %s %d > 32", who, name, v);
    return ANTSRL_OK;
}

int antsrl_check_D(const char *who, int32_t n_features, int32_t agent_dim, int32_t mem_size)
{
    const long long D = (long long)n_features + agent_dim + mem_size;
    if (D > 1024) return fail(ANTSRL_E_UNSUPPORTED, "%s: D = n_features + agent_dim + mem_size = %lld > 1024", who, D);
    return ANTSRL_OK;
}

static int check_width(const char *who, const char *name, int32_t v)
{
    if (v < 1) return fail(ANTSRL_E_INVALID, "%s: %s must be >= 1 (%d)", who, name, v);
    return antsrl_check_max32(who, name, v);
}

int antsrl_check_epsilon(const char *who, int member, double epsilon)
{
    if (epsilon >= 0.0 && epsilon <= 1.0) return ANTSRL_OK;
    if (member < 0) return fail(ANTSRL_E_INVALID, "%s: epsilon must be in [0, 1] (%g)", who, epsilon);
    return fail(ANTSRL_E_INVALID, "%s: member %d: epsilon must be in [0, 1] (%g)", who, member, epsilon);
}

int antsrl_check_obs_format(const char *who, int obs_format)
{
    if (obs_format != ANTSRL_OBS_F32 && obs_format != ANTSRL_OBS_BF16)
        return fail(ANTSRL_E_INVALID, "%s: obs_format must be ANTSRL_OBS_F32 or ANTSRL_OBS_BF16 (%d)", who, obs_format);
    return ANTSRL_OK;
}

void antsrl_sel_args(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants, double epsilon,
                     int32_t n_rot, int32_t n_ph, SelArgs *a)
{
    *a = SelArgs{};
    a->seed = seed; a->step = step; a->epsilon = epsilon;
    a->env_base = (uint32_t)env_id_base; a->n_ants = (uint32_t)n_ants; a->n_rot = (uint32_t)n_rot; a->n_ph = (uint32_t)n_ph;
    a->M = (uint32_t)((long long)n_envs * n_ants);
}

int antsrl_ring_rows(const char *who, const char *rows_words, long long rows, int64_t K, int64_t head, int64_t max_len,
                     RecArgs *a)
{
    if (K < 1 || K > rows)
        return fail(ANTSRL_E_INVALID, "%s: K must be in [1, %s = %lld] (%lld)", who, rows_words, rows, (long long)K);
    if (max_len < 1 || max_len > (1LL << 40)) return fail(ANTSRL_E_INVALID, "%s: max_len must be in [1, 2^40] (%lld)", who, (long long)max_len);
    if (head < 0 || head >= max_len)
        return fail(ANTSRL_E_INVALID, "%s: head must be in [0, max_len = %lld) (%lld)", who, (long long)max_len, (long long)head);
    a->K = K;
    a->n_write = K < max_len ? K : max_len; // only the newest max_len entries can survive
    a->j0 = K - a->n_write;
    a->row0 = (head + a->j0) % max_len;
    a->max_len = max_len;
    return ANTSRL_OK;
}

int antsrl_rec_pre(const char *who, RecArgs *a, bool obs_bf16, const void *obs, const float *agent_state, const float *memory,
                   const int8_t *rotation, const int8_t *pheromone, float *states, float *agent_states, int64_t *actions)
{
    REQUIRE(obs, obs_bf16 ? 2 : 4);
    REQUIRE(agent_state, 4);
    if (a->mem > 0) REQUIRE(memory, 4);
    REQUIRE(rotation, 1);
    REQUIRE(states, 4);
    REQUIRE(agent_states, 4);
    REQUIRE(actions, 8);
    a->obs = obs; a->agent_state = agent_state; a->memory = memory; a->rot = rotation; a->ph = pheromone;
    a->states = states; a->agent_states = agent_states; a->actions = actions;
    return ANTSRL_OK;
}

int antsrl_rec_post(const char *who, RecArgs *a, bool obs_bf16, const void *obs, const float *agent_state, const float *memory,
                    const float *reward, const uint8_t *done, float *rewards, float *new_states, float *new_agent_states,
                    uint8_t *dones)
{
    REQUIRE(obs, obs_bf16 ? 2 : 4);
    REQUIRE(agent_state, 4);
    if (a->mem > 0) REQUIRE(memory, 4);
    REQUIRE(reward, 4);
    REQUIRE(done, 1);
    REQUIRE(rewards, 4);
    REQUIRE(new_states, 4);
    REQUIRE(new_agent_states, 4);
    REQUIRE(dones, 1);
    a->obs = obs; a->agent_state = agent_state; a->memory = memory; a->reward = reward; a->done = done;
    a->rewards = rewards; a->states = new_states; a->agent_states = new_agent_states; a->dones = dones;
    return ANTSRL_OK;
}

// ---- select and plan
#define MISALIGNED(p, n) (((uintptr_t)(p) & ((n) - 1)) != 0)

extern "C" int antsrl_agent_select(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants,
                                   double epsilon, int32_t n_rot, int32_t n_ph, int32_t mem_size, int8_t *rotation,
                                   int8_t *pheromone, const float *mem_old, float *mem_next, uint8_t *explored, void *stream)
{
    const char *who = "agent_select";
    int rc = antsrl_check_batch(who, env_id_base, n_envs, n_ants);
    if (rc == ANTSRL_OK) rc = check_width(who, "n_rot", n_rot);
    if (rc == ANTSRL_OK) rc = check_width(who, "n_ph", n_ph);
    if (rc == ANTSRL_OK) rc = check_width(who, "mem_size", mem_size);
    if (rc == ANTSRL_OK) rc = antsrl_check_epsilon(who, -1, epsilon);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(rotation, 1);
    REQUIRE(pheromone, 1);
    REQUIRE(mem_old, 1);
    REQUIRE(mem_next, 1);
    if (MISALIGNED(mem_old, 4) || MISALIGNED(mem_next, 4)) return fail(ANTSRL_E_INVALID, "%s: mem_old and mem_next must be 4-byte aligned", who);
    if (mem_old != mem_next) { // the same buffer, or two that do not touch
        const uintptr_t o = (uintptr_t)mem_old, n = (uintptr_t)mem_next;
        const uintptr_t bytes = (uintptr_t)n_envs * (uintptr_t)n_ants * (uintptr_t)mem_size * 4;
        if (o < n + bytes && n < o + bytes) return fail(ANTSRL_E_INVALID, "%s: mem_old and mem_next overlap without being equal", who);
    }
    SelArgs a;
    antsrl_sel_args(seed, step, env_id_base, n_envs, n_ants, epsilon, n_rot, n_ph, &a);
    a.rot = rotation; a.ph = pheromone; a.mem_old = mem_old; a.mem_next = mem_next; a.explored = explored;
    const uint64_t env_floats = (uint64_t)n_ants * (uint64_t)mem_size;
    const bool vec = env_floats % 4 == 0 && !MISALIGNED(mem_old, 16) && !MISALIGNED(mem_next, 16);
    const uint64_t env_elems = vec ? env_floats / 4 : env_floats;
    if (env_elems > 0xffffffffULL) return fail(ANTSRL_E_UNSUPPORTED, "%s: n_ants * mem_size = %llu is too large", who, (unsigned long long)env_floats);
    a.env_elems = (uint32_t)env_elems;
    a.mem_elems = env_elems * (uint64_t)n_envs;
    return enqueued(antsrl_launch_agent_select(a, vec, (hipStream_t)stream), who);
}

extern "C" int antsrl_agent_plan(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants,
                                 double epsilon, int32_t *tiles, int32_t *n_live, void *stream)
{
    const char *who = "agent_plan";
    int rc = antsrl_check_batch(who, env_id_base, n_envs, n_ants);
    if (rc == ANTSRL_OK) rc = antsrl_check_epsilon(who, -1, epsilon);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(tiles, 4);
    REQUIRE(n_live, 4);
    SelArgs a;
    antsrl_sel_args(seed, step, env_id_base, n_envs, n_ants, epsilon, 0, 0, &a);
    return enqueued(antsrl_launch_agent_plan(a, tiles, n_live, (hipStream_t)stream), who);
}

// the memory-less select (the linear agent: agents/collect_agent.py:161-177): the kernel copies no memory when
// mem_old == mem_next, both NULL here
extern "C" int antsrl_agent_select_actions(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants,
                                           double epsilon, int32_t n_rot, int32_t n_ph, int8_t *rotation, int8_t *pheromone,
                                           uint8_t *explored, void *stream)
{
    const char *who = "agent_select_actions";
    int rc = antsrl_check_batch(who, env_id_base, n_envs, n_ants);
    if (rc == ANTSRL_OK) rc = check_width(who, "n_rot", n_rot);
    if (rc == ANTSRL_OK) rc = check_width(who, "n_ph", n_ph);
    if (rc == ANTSRL_OK) rc = antsrl_check_epsilon(who, -1, epsilon);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(rotation, 1);
    REQUIRE(pheromone, 1);
    SelArgs a;
    antsrl_sel_args(seed, step, env_id_base, n_envs, n_ants, epsilon, n_rot, n_ph, &a);
    a.rot = rotation; a.ph = pheromone; a.explored = explored;
    return enqueued(antsrl_launch_agent_select(a, false, (hipStream_t)stream), who);
}

// ---- record
// *a = the record kernel's arguments of spec *r, or the refusal.  plain: the memory-less entries, whose spec has
// mem_size == 0 (the entries with a memory go on refusing that); the record kernel's small fields are agent_dim +
// mem_size wide, so with mem_size 0 it never touches a memory pointer
static int rec_spec(const char *who, const AntsRecordSpec *r, bool plain, RecArgs *a)
{
    if (!r) return fail(ANTSRL_E_INVALID, "%s: NULL spec", who);
    int rc = antsrl_check_batch(who, r->env_id_base, r->n_envs, r->n_ants);
    if (rc != ANTSRL_OK) return rc;
    if (r->n_features < 1) return fail(ANTSRL_E_INVALID, "%s: n_features must be >= 1 (%d)", who, r->n_features);
    if ((rc = check_width(who, "agent_dim", r->agent_dim)) != ANTSRL_OK) return rc;
    if (plain && r->mem_size != 0) return fail(ANTSRL_E_INVALID, "%s: mem_size must be 0 (%d): this entry records no memory", who, r->mem_size);
    if (!plain && (rc = check_width(who, "mem_size", r->mem_size)) != ANTSRL_OK) return rc;
    if ((rc = check_width(who, "n_rot", r->n_rot)) != ANTSRL_OK) return rc;
    if ((rc = antsrl_check_D(who, r->n_features, r->agent_dim, r->mem_size)) != ANTSRL_OK) return rc;
    if ((rc = antsrl_check_obs_format(who, r->obs_format)) != ANTSRL_OK) return rc;
    if (r->obs_pitch != 0 && (r->obs_pitch < r->n_features || r->obs_pitch >= (1 << 24)))
        return fail(ANTSRL_E_INVALID, "%s: obs_pitch %d: 0 (dense) or at least the row's %d elements (and below 2^24)", who,
                    r->obs_pitch, r->n_features);
    a->M = (long long)r->n_envs * r->n_ants;
    if ((rc = antsrl_ring_rows(who, "n_envs * n_ants", a->M, r->K, r->head, r->max_len, a)) != ANTSRL_OK) return rc;
    a->seed = r->seed; a->step = r->step; a->env_base = (uint64_t)r->env_id_base;
    a->pitch = r->obs_pitch ? r->obs_pitch : r->n_features;
    a->n_ants = r->n_ants; a->F = r->n_features; a->A = r->agent_dim; a->mem = r->mem_size; a->half_rot = r->n_rot / 2;
    return ANTSRL_OK;
}

// an entry: the spec, the half's pointers (memory NULL for the plain entries), the launch
static int launch_rec(const char *who, const AntsRecordSpec *r, const RecArgs &a, bool post, void *stream)
{
    return enqueued(antsrl_launch_replay_record(a, r->obs_format == ANTSRL_OBS_BF16, post, (hipStream_t)stream), who);
}

extern "C" int antsrl_replay_record_pre(const AntsRecordSpec *r, const void *obs, const float *agent_state,
                                        const float *memory, const int8_t *rotation, const int8_t *pheromone, float *states,
                                        float *agent_states, int64_t *actions, void *stream)
{
    const char *who = "replay_record_pre";
    RecArgs a = {};
    int rc = rec_spec(who, r, false, &a);
    if (rc == ANTSRL_OK)
        rc = antsrl_rec_pre(who, &a, r->obs_format == ANTSRL_OBS_BF16, obs, agent_state, memory, rotation, pheromone, states,
                            agent_states, actions);
    return rc != ANTSRL_OK ? rc : launch_rec(who, r, a, false, stream);
}

extern "C" int antsrl_replay_record_post(const AntsRecordSpec *r, const void *obs, const float *agent_state,
                                         const float *memory, const float *reward, const uint8_t *done, float *rewards,
                                         float *new_states, float *new_agent_states, uint8_t *dones, void *stream)
{
    const char *who = "replay_record_post";
    RecArgs a = {};
    int rc = rec_spec(who, r, false, &a);
    if (rc == ANTSRL_OK)
        rc = antsrl_rec_post(who, &a, r->obs_format == ANTSRL_OBS_BF16, obs, agent_state, memory, reward, done, rewards,
                             new_states, new_agent_states, dones);
    return rc != ANTSRL_OK ? rc : launch_rec(who, r, a, true, stream);
}

extern "C" int antsrl_replay_record_pre_plain(const AntsRecordSpec *r, const void *obs, const float *agent_state,
                                              const int8_t *rotation, const int8_t *pheromone, float *states,
                                              float *agent_states, int64_t *actions, void *stream)
{
    const char *who = "replay_record_pre_plain";
    RecArgs a = {};
    int rc = rec_spec(who, r, true, &a);
    if (rc == ANTSRL_OK)
        rc = antsrl_rec_pre(who, &a, r->obs_format == ANTSRL_OBS_BF16, obs, agent_state, nullptr, rotation, pheromone, states,
                            agent_states, actions);
    return rc != ANTSRL_OK ? rc : launch_rec(who, r, a, false, stream);
}

extern "C" int antsrl_replay_record_post_plain(const AntsRecordSpec *r, const void *obs, const float *agent_state,
                                               const float *reward, const uint8_t *done, float *rewards, float *new_states,
                                               float *new_agent_states, uint8_t *dones, void *stream)
{
    const char *who = "replay_record_post_plain";
    RecArgs a = {};
    int rc = rec_spec(who, r, true, &a);
    if (rc == ANTSRL_OK)
        rc = antsrl_rec_post(who, &a, r->obs_format == ANTSRL_OBS_BF16, obs, agent_state, nullptr, reward, done, rewards,
                             new_states, new_agent_states, dones);
    return rc != ANTSRL_OK ? rc : launch_rec(who, r, a, true, stream);
}
