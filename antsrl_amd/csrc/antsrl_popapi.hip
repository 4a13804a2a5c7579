// antsrl_popapi.hip — the population of linear agents in the C-ABI of libantsrl_hip.so (include/antsrl.h, "The population
// of linear agents"): antsrl_pop_policy / _select / _record_pre / _record_post / _lintrain_step in front of
// antsrl_population.hip's kernels.
//
// Host-side only: validates every argument before any HIP call and enqueues on the caller's stream.  No handle, no
// allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_adam.h"
#include "antsrl_device.h"
#include "antsrl_dqn.h"
#include "antsrl_fail.h"
#include "antsrl_policy_flat.h"
#include "antsrl_population.h"

#define POP_N_ROT 3 // the linear net's heads are 3 wide
#define POP_N_PH 3
#define POP_AGENT_DIM 2

// what every entry checks of its spec; fills the table's seeds and epsilons and *Em, the environments per member
static int pop_spec(const char *who, const AntsPopSpec *s, PopTable *t, int *Em)
{
    if (!s) return fail(ANTSRL_E_INVALID, "%s: NULL spec", who);
    if (s->n_members < 1 || s->n_members > ANTSRL_POP_MAX)
        return fail(ANTSRL_E_INVALID, "%s: n_members must be in [1, ANTSRL_POP_MAX = %d] (%d)", who, ANTSRL_POP_MAX, s->n_members);
    int rc = antsrl_check_batch(who, s->env_id_base, s->n_envs, s->n_ants);
    if (rc != ANTSRL_OK) return rc;
    if (s->n_envs % s->n_members)
        return fail(ANTSRL_E_INVALID, "%s: n_envs = %d is not a multiple of n_members = %d (members own equal shares)", who,
                    s->n_envs, s->n_members);
    if (s->n_features < 1) return fail(ANTSRL_E_INVALID, "%s: n_features must be >= 1 (%d)", who, s->n_features);
    if (s->n_features + 2 > 1024) return fail(ANTSRL_E_UNSUPPORTED, "%s: n_features + 2 = %d > 1024", who, s->n_features + 2);
    if (s->obs_format != ANTSRL_OBS_F32 && s->obs_format != ANTSRL_OBS_BF16)
        return fail(ANTSRL_E_INVALID, "%s: obs_format must be ANTSRL_OBS_F32 or ANTSRL_OBS_BF16 (%d)", who, s->obs_format);
    if (s->obs_pitch != 0 && s->obs_pitch != s->n_features)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: a population reads dense observation rows: obs_pitch %d must be 0 or n_features = %d",
                    who, s->obs_pitch, s->n_features);
    for (int p = 0; p < s->n_members; ++p) {
        const AntsPopMember &m = s->members[p];
        if (!(m.epsilon >= 0.0 && m.epsilon <= 1.0))
            return fail(ANTSRL_E_INVALID, "%s: member %d: epsilon must be in [0, 1] (%g)", who, p, m.epsilon);
        if (!(m.discount == m.discount)) return fail(ANTSRL_E_INVALID, "%s: member %d: discount is NaN", who, p);
        t->m[p].seed = m.seed;
        t->m[p].epsilon = m.epsilon;
        t->m[p].discount = m.discount;
        t->m[p].step_size = 0.0f;
    }
    *Em = s->n_envs / s->n_members;
    return ANTSRL_OK;
}

// The acting kernel's rule: its producer loads 16-byte pieces from the first byte of a member's rows, so every member's
// slice must start 16-byte aligned: obs itself, and Em * n_ants * n_features * sizeof(element) a multiple of 16.
static int pop_flat_rule(const char *who, const AntsPopSpec *s, int Em)
{
    if (!pol_flat_fits(s->n_features))
        return fail(ANTSRL_E_UNSUPPORTED, "%s: n_features = %d: the net and two 32-row images do not fit the LDS, and a population "
                                          "acts with the flat form only", who, s->n_features);
    const long long bytes = (long long)Em * s->n_ants * s->n_features * (s->obs_format == ANTSRL_OBS_BF16 ? 2 : 4);
    if (bytes % 16)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: a member's observation slice of %lld bytes (n_envs / n_members * n_ants * n_features "
                                          "* sizeof(element)) must be a multiple of 16: members' rows start 16-byte aligned", who, bytes);
    return ANTSRL_OK;
}

extern "C" int antsrl_pop_policy(const AntsPopSpec *s, const void *obs, const float *agent_state, const float *w1,
                                 const float *b1, const float *heads, const float *target_l3, int8_t *rotation,
                                 int8_t *pheromone, void *stream)
{
    const char *who = "pop_policy";
    PopTable t;
    int Em = 0;
    int rc = pop_spec(who, s, &t, &Em);
    if (rc == ANTSRL_OK) rc = pop_flat_rule(who, s, Em);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(obs, 16);
    REQUIRE(agent_state, 4);
    REQUIRE(w1, 4);
    REQUIRE(b1, 4);
    REQUIRE(heads, 4);
    REQUIRE(target_l3, 4);
    REQUIRE(rotation, 1);
    REQUIRE(pheromone, 1);
    PopPolicyArgs a;
    a.obs = obs; a.agent_state = agent_state; a.w1 = w1; a.b1 = b1; a.heads = heads; a.target_l3 = target_l3;
    a.rot = rotation; a.ph = pheromone;
    a.Mm = Em * s->n_ants; a.F = s->n_features; a.P = s->n_members;
    return enqueued(antsrl_launch_pop_policy(a, s->obs_format == ANTSRL_OBS_BF16, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_select(const AntsPopSpec *s, uint64_t step, int8_t *rotation, int8_t *pheromone, uint8_t *explored,
                                 void *stream)
{
    const char *who = "pop_select";
    PopTable t;
    int Em = 0;
    const int rc = pop_spec(who, s, &t, &Em);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(rotation, 1);
    REQUIRE(pheromone, 1);
    SelArgs a = {};
    a.step = step;
    a.rot = rotation; a.ph = pheromone; a.explored = explored; // mem_old == mem_next == NULL: no memory part
    a.env_base = (uint32_t)s->env_id_base; a.n_ants = (uint32_t)s->n_ants; a.n_rot = POP_N_ROT; a.n_ph = POP_N_PH;
    a.M = (uint32_t)(Em * s->n_ants);
    return enqueued(antsrl_launch_pop_select(a, t, s->n_members, Em, (hipStream_t)stream), who);
}

// the ring's part of a record entry: K rows per member into the rows behind `head` of every member's slab
static int pop_rec(const char *who, const AntsPopSpec *s, int Em, uint64_t step, int64_t K, int64_t head, int64_t max_len,
                   RecArgs *a)
{
    const long long Mm = (long long)Em * s->n_ants;
    if (K < 1 || K > Mm)
        return fail(ANTSRL_E_INVALID, "%s: K must be in [1, n_envs / n_members * n_ants = %lld] (%lld)", who, Mm, (long long)K);
    if (max_len < 1 || max_len > (1LL << 40)) return fail(ANTSRL_E_INVALID, "%s: max_len must be in [1, 2^40] (%lld)", who, (long long)max_len);
    if (head < 0 || head >= max_len)
        return fail(ANTSRL_E_INVALID, "%s: head must be in [0, max_len = %lld) (%lld)", who, (long long)max_len, (long long)head);
    a->step = step; a->env_base = (uint64_t)s->env_id_base;
    a->M = Mm; a->K = K;
    a->n_write = K < max_len ? K : max_len; // only the newest max_len entries can survive
    a->j0 = K - a->n_write;
    a->row0 = (head + a->j0) % max_len;
    a->max_len = max_len;
    a->pitch = s->n_features;
    a->n_ants = s->n_ants; a->F = s->n_features; a->A = POP_AGENT_DIM; a->mem = 0; a->half_rot = POP_N_ROT / 2;
    return ANTSRL_OK;
}

extern "C" int antsrl_pop_record_pre(const AntsPopSpec *s, uint64_t step, int64_t K, int64_t head, int64_t max_len,
                                     const void *obs, const float *agent_state, const int8_t *rotation,
                                     const int8_t *pheromone, float *states, float *agent_states, int64_t *actions,
                                     void *stream)
{
    const char *who = "pop_record_pre";
    PopTable t;
    int Em = 0;
    RecArgs a = {};
    int rc = pop_spec(who, s, &t, &Em);
    if (rc == ANTSRL_OK) rc = pop_rec(who, s, Em, step, K, head, max_len, &a);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(obs, s->obs_format == ANTSRL_OBS_BF16 ? 2 : 4);
    REQUIRE(agent_state, 4);
    REQUIRE(rotation, 1);
    REQUIRE(states, 4);
    REQUIRE(agent_states, 4);
    REQUIRE(actions, 8);
    a.obs = obs; a.agent_state = agent_state; a.rot = rotation; a.ph = pheromone;
    a.states = states; a.agent_states = agent_states; a.actions = actions;
    return enqueued(antsrl_launch_pop_record(a, t, s->n_members, Em, s->obs_format == ANTSRL_OBS_BF16, false, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_record_post(const AntsPopSpec *s, uint64_t step, int64_t K, int64_t head, int64_t max_len,
                                      const void *obs, const float *agent_state, const float *reward, const uint8_t *done,
                                      float *rewards, float *new_states, float *new_agent_states, uint8_t *dones,
                                      void *stream)
{
    const char *who = "pop_record_post";
    PopTable t;
    int Em = 0;
    RecArgs a = {};
    int rc = pop_spec(who, s, &t, &Em);
    if (rc == ANTSRL_OK) rc = pop_rec(who, s, Em, step, K, head, max_len, &a);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(obs, s->obs_format == ANTSRL_OBS_BF16 ? 2 : 4);
    REQUIRE(agent_state, 4);
    REQUIRE(reward, 4);
    REQUIRE(done, 1);
    REQUIRE(rewards, 4);
    REQUIRE(new_states, 4);
    REQUIRE(new_agent_states, 4);
    REQUIRE(dones, 1);
    a.obs = obs; a.agent_state = agent_state; a.reward = reward; a.done = done;
    a.rewards = rewards; a.states = new_states; a.agent_states = new_agent_states; a.dones = dones;
    return enqueued(antsrl_launch_pop_record(a, t, s->n_members, Em, s->obs_format == ANTSRL_OBS_BF16, true, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_lintrain_step(const AntsPopSpec *s, const float *w1, const float *b1, float *heads,
                                        const float *target_l3, float *adam, const float *states, const float *agent_states,
                                        const int64_t *actions, const float *rewards, const float *new_states,
                                        const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx,
                                        int64_t B, int64_t step, double beta1, double beta2, double eps, float *grads,
                                        float *loss, double *running_loss, int first_loss, void *stream)
{
    const char *who = "pop_lintrain_step";
    PopTable t;
    int Em = 0;
    int rc = pop_spec(who, s, &t, &Em);
    if (rc != ANTSRL_OK) return rc;
    if (B < 1) return fail(ANTSRL_E_INVALID, "%s: B must be >= 1 (%lld)", who, (long long)B);
    if (B > 32 * LT_FUSED_TILES)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: B = %lld > %d rows: a member's step is one workgroup", who, (long long)B, 32 * LT_FUSED_TILES);
    REQUIRE(w1, 4);
    REQUIRE(b1, 4);
    REQUIRE(heads, 4);
    REQUIRE(target_l3, 4);
    REQUIRE(adam, 4);
    REQUIRE(idx, 8);
    LinTrainArgs a = {};
    // member 0's minibatch: the slab's arrays, idx, grads, loss (the discount comes from the table)
    rc = antsrl_dqn_minibatch(who, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows, idx, B,
                              0.0f, grads, false, loss, &a.batch);
    if (rc != ANTSRL_OK) return rc;
    if ((uintptr_t)running_loss & 7) return fail(ANTSRL_E_INVALID, "%s: running_loss must be 8-byte aligned", who);
    for (int p = 0; p < s->n_members; ++p) { // Adam's scalars per member: the step size is the learning rate's
        if ((rc = antsrl_adam_args(who, step, s->members[p].learning_rate, beta1, beta2, eps, &a.adam)) != ANTSRL_OK) return rc;
        t.m[p].step_size = a.adam.step_size;
    }
    const int F = s->n_features;
    a.batch.F = F; a.batch.ksteps = (F + 15) / 16; a.batch.ntiles = ((int)B + 31) / 32;
    a.batch.dq_scale = (float)(2.0 / (3.0 * (double)B));
    a.batch.loss_scale = (float)(1.0 / (3.0 * (double)B));
    a.w1 = w1; a.b1 = b1; a.heads = heads; a.target_l3 = target_l3;
    a.adam.m = adam; a.adam.v = adam + LT_HEADS;
    const PopRunningLoss rl = {running_loss, first_loss != 0};
    return enqueued(antsrl_launch_pop_lintrain(a, t, s->n_members, rl, (hipStream_t)stream), who);
}
