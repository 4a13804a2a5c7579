// antsrl_popapi.hip — the populations in the C-ABI of libantsrl_hip.so (include/antsrl.h, "The population of ..."), one
// line per population: its entries, and the file of the kernels they stand in front of.
//   linear agents   antsrl_pop_policy / _select / _record_pre / _record_post / _lintrain_step        antsrl_population.hip
//   explore agents  antsrl_pop_explore_policy / antsrl_pop_exptrain_sizes / _step (select and        antsrl_popexplore.hip
//                   record are the linear agents': no pheromone head, and the ring stores none)
//   joint agents    antsrl_pop_joint_policy / antsrl_pop_jointtrain_sizes / _step (likewise)         antsrl_popjoint.hip
//   memory nets     antsrl_pop_memtrain_sizes / _step                                                antsrl_popmemtrain.hip
//   memory agents   antsrl_pop_memnet_sizes / antsrl_pop_policy_memory                               antsrl_popmemnet.hip
//                   antsrl_pop_memory_select / _record_pre / _record_post (with the carried memory)  antsrl_population.hip
//   rework agents   antsrl_pop_rework_collapse / antsrl_pop_policy_rework / _select /                antsrl_poprework.hip
//                   antsrl_pop_reworktrain_sizes / _step (select without the fusion and record
//                   are the linear agents')
//   every kind      antsrl_pop_fitness (a member's episode reward off the monitor's block)           antsrl_popfitness.hip
//                   antsrl_pop_exploit (members' rows over other members', one launch)               antsrl_checkpoint.hip
//
// Host-side only: validates every argument before any HIP call and enqueues on the caller's stream.  No handle, no
// allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "antsrl_adam.h"
#include "antsrl_checkpoint.h" // EnvCopyTable: the exploit is k_env_copy's
#include "antsrl_device.h"
#include "antsrl_dqn.h"
#include "antsrl_fail.h"
#include "antsrl_launch.h" // antsrl_launch_env_copy
#include "antsrl_loopapi.h"
#include "antsrl_memnet.h"
#include "antsrl_policy_flat.h"
#include "antsrl_population.h"
#include "antsrl_reworkapi.h" // rework_check

#define POP_N_ROT 3 // the linear net's heads are 3 wide
#define POP_N_PH 3
#define POP_AGENT_DIM 2
#define POP_L1T_LIMIT "at most four forward workgroups" // (what Net::POP_MAX_B rows are, antsrl_l1train.h)

static int pop_n_members(const char *who, int n_members)
{
    if (n_members >= 1 && n_members <= ANTSRL_POP_MAX) return ANTSRL_OK;
    return fail(ANTSRL_E_INVALID, "%s: n_members must be in [1, ANTSRL_POP_MAX = %d] (%d)", who, ANTSRL_POP_MAX, n_members);
}

// what every entry checks of its spec; fills the table's seeds and epsilons and *Em, the environments per member
static int pop_spec(const char *who, const AntsPopSpec *s, PopTable *t, int *Em)
{
    if (!s) return fail(ANTSRL_E_INVALID, "%s: NULL spec", who);
    int rc = pop_n_members(who, s->n_members);
    if (rc == ANTSRL_OK) rc = antsrl_check_batch(who, s->env_id_base, s->n_envs, s->n_ants);
    if (rc != ANTSRL_OK) return rc;
    if (s->n_envs % s->n_members)
        return fail(ANTSRL_E_INVALID, "%s: n_envs = %d is not a multiple of n_members = %d (members own equal shares)", who,
                    s->n_envs, s->n_members);
    if ((rc = lt_features(who, s->n_features)) != ANTSRL_OK) return rc;
    if ((rc = antsrl_check_obs_format(who, s->obs_format)) != ANTSRL_OK) return rc;
    if (s->obs_pitch != 0 && s->obs_pitch != s->n_features)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: a population reads dense observation rows: obs_pitch %d must be 0 or n_features = %d",
                    who, s->obs_pitch, s->n_features);
    for (int p = 0; p < s->n_members; ++p) {
        const AntsPopMember &m = s->members[p];
        if ((rc = antsrl_check_epsilon(who, p, m.epsilon)) != ANTSRL_OK) return rc;
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
static int pop_slice_rule(const char *who, const AntsPopSpec *s, int Em);
static int pop_flat_rule(const char *who, const AntsPopSpec *s, int Em)
{
    if (!pol_flat_fits(s->n_features))
        return fail(ANTSRL_E_UNSUPPORTED, "%s: n_features = %d: the net and two 32-row images do not fit the LDS, and a population "
                                          "acts with the flat form only", who, s->n_features);
    return pop_slice_rule(who, s, Em);
}

// pop_flat_rule's alignment rule alone, for an acting kernel that is not the flat form (the rework net's, which reads
// its rows by 16-byte and dword loads from a member's first byte)
static int pop_slice_rule(const char *who, const AntsPopSpec *s, int Em)
{
    const long long bytes = (long long)Em * s->n_ants * s->n_features * (s->obs_format == ANTSRL_OBS_BF16 ? 2 : 4);
    if (bytes % 16)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: a member's observation slice of %lld bytes (n_envs / n_members * n_ants * n_features "
                                          "* sizeof(element)) must be a multiple of 16: members' rows start 16-byte aligned", who, bytes);
    return ANTSRL_OK;
}

// the front of the three flat acting entries: the spec's rules, the acting kernel's, then the rows; fills *Em
static int pop_flat_policy(const char *who, const AntsPopSpec *s, const void *obs, const float *agent_state, int *Em)
{
    PopTable t;
    int rc = pop_spec(who, s, &t, Em);
    if (rc == ANTSRL_OK) rc = pop_flat_rule(who, s, *Em);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(obs, 16);
    REQUIRE(agent_state, 4);
    return ANTSRL_OK;
}

extern "C" int antsrl_pop_policy(const AntsPopSpec *s, const void *obs, const float *agent_state, const float *w1,
                                 const float *b1, const float *heads, const float *target_l3, int8_t *rotation,
                                 int8_t *pheromone, void *stream)
{
    const char *who = "pop_policy";
    int Em = 0;
    const int rc = pop_flat_policy(who, s, obs, agent_state, &Em);
    if (rc != ANTSRL_OK) return rc;
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
    SelArgs a; // member 0's Em environments; seed and epsilon come from the table
    antsrl_sel_args(0, step, s->env_id_base, Em, s->n_ants, 0.0, POP_N_ROT, POP_N_PH, &a);
    a.rot = rotation; a.ph = pheromone; a.explored = explored;
    return enqueued(antsrl_launch_pop_select(a, t, s->n_members, Em, (hipStream_t)stream), who);
}

static int pop_mem_spec(const char *who, const AntsPopSpec *s, const AntsMemNetShape *shape, PopTable *t, int *Em, MemNetDims *d,
                        size_t *pack_stride); // (with the memory agents' entries, below)

// The front of a record entry: the spec's rules, and with with_memory the shape's (pop_mem_spec), then RecArgs for member
// 0: K rows per member into the rows behind `head` of every member's slab.  With a memory, agent_states rows are
// agent_dim + mem_size wide.
static int pop_rec(const char *who, const AntsPopSpec *s, bool with_memory, const AntsMemNetShape *shape, uint64_t step, int64_t K,
                   int64_t head, int64_t max_len, PopTable *t, int *Em, RecArgs *a)
{
    MemNetDims d;
    size_t stride = 0;
    int rc = with_memory ? pop_mem_spec(who, s, shape, t, Em, &d, &stride) : pop_spec(who, s, t, Em);
    if (rc != ANTSRL_OK) return rc;
    a->M = (long long)*Em * s->n_ants;
    rc = antsrl_ring_rows(who, "n_envs / n_members * n_ants", a->M, K, head, max_len, a);
    if (rc != ANTSRL_OK) return rc;
    a->step = step; a->env_base = (uint64_t)s->env_id_base;
    a->pitch = s->n_features;
    a->n_ants = s->n_ants; a->F = s->n_features; a->A = POP_AGENT_DIM; a->mem = 0; a->half_rot = POP_N_ROT / 2;
    if (with_memory) { a->A = d.A; a->mem = d.mem; a->half_rot = d.n_rot / 2; }
    return ANTSRL_OK;
}

// antsrl_pop_record_pre and antsrl_pop_memory_record_pre (with_memory: shape and memory are theirs; else NULL)
static int pop_record_pre(const char *who, const AntsPopSpec *s, bool with_memory, const AntsMemNetShape *shape, uint64_t step,
                          int64_t K, int64_t head, int64_t max_len, const void *obs, const float *agent_state, const float *memory,
                          const int8_t *rotation, const int8_t *pheromone, float *states, float *agent_states, int64_t *actions,
                          void *stream)
{
    PopTable t;
    int Em = 0;
    RecArgs a = {};
    int rc = pop_rec(who, s, with_memory, shape, step, K, head, max_len, &t, &Em, &a);
    if (rc != ANTSRL_OK) return rc;
    const bool bf16 = s->obs_format == ANTSRL_OBS_BF16;
    rc = antsrl_rec_pre(who, &a, bf16, obs, agent_state, memory, rotation, pheromone, states, agent_states, actions);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(antsrl_launch_pop_record(a, t, s->n_members, Em, bf16, false, (hipStream_t)stream), who);
}

// antsrl_pop_record_post and antsrl_pop_memory_record_post, likewise
static int pop_record_post(const char *who, const AntsPopSpec *s, bool with_memory, const AntsMemNetShape *shape, uint64_t step,
                           int64_t K, int64_t head, int64_t max_len, const void *obs, const float *agent_state,
                           const float *memory, const float *reward, const uint8_t *done, float *rewards, float *new_states,
                           float *new_agent_states, uint8_t *dones, void *stream)
{
    PopTable t;
    int Em = 0;
    RecArgs a = {};
    int rc = pop_rec(who, s, with_memory, shape, step, K, head, max_len, &t, &Em, &a);
    if (rc != ANTSRL_OK) return rc;
    const bool bf16 = s->obs_format == ANTSRL_OBS_BF16;
    rc = antsrl_rec_post(who, &a, bf16, obs, agent_state, memory, reward, done, rewards, new_states, new_agent_states, dones);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(antsrl_launch_pop_record(a, t, s->n_members, Em, bf16, true, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_record_pre(const AntsPopSpec *s, uint64_t step, int64_t K, int64_t head, int64_t max_len,
                                     const void *obs, const float *agent_state, const int8_t *rotation,
                                     const int8_t *pheromone, float *states, float *agent_states, int64_t *actions,
                                     void *stream)
{
    return pop_record_pre("pop_record_pre", s, false, nullptr, step, K, head, max_len, obs, agent_state, nullptr, rotation, pheromone,
                          states, agent_states, actions, stream);
}

extern "C" int antsrl_pop_record_post(const AntsPopSpec *s, uint64_t step, int64_t K, int64_t head, int64_t max_len,
                                      const void *obs, const float *agent_state, const float *reward, const uint8_t *done,
                                      float *rewards, float *new_states, float *new_agent_states, uint8_t *dones,
                                      void *stream)
{
    return pop_record_post("pop_record_post", s, false, nullptr, step, K, head, max_len, obs, agent_state, nullptr, reward, done,
                           rewards, new_states, new_agent_states, dones, stream);
}

// The training entries refuse in the order spec, B (antsrl_dqn_B, antsrl_dqn.h, told what of the entry's step its limit
// is), their pointers, dqn_batch's arguments, running_loss, Adam's.

// running_loss's alignment, then Adam's scalars per member: the step size is the learning rate's and goes into the table
static int pop_train_tail(const char *who, const AntsPopSpec *s, int64_t step, double beta1, double beta2, double eps,
                          const double *running_loss, AdamArgs *adam, PopTable *t)
{
    if ((uintptr_t)running_loss & 7) return fail(ANTSRL_E_INVALID, "%s: running_loss must be 8-byte aligned", who);
    for (int p = 0; p < s->n_members; ++p) {
        const int rc = antsrl_adam_args(who, step, s->members[p].learning_rate, beta1, beta2, eps, adam);
        if (rc != ANTSRL_OK) return rc;
        t->m[p].step_size = adam->step_size;
    }
    return ANTSRL_OK;
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
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, 32 * LT_FUSED_TILES, "one workgroup");
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(w1, 4);
    REQUIRE(b1, 4);
    REQUIRE(heads, 4);
    REQUIRE(target_l3, 4);
    REQUIRE(adam, 4);
    REQUIRE(idx, 8);
    LinTrainArgs a = {};
    // member 0's minibatch: the slab's arrays, idx, grads, loss (the discount comes from the table), no workspace
    rc = dqn_batch(who, s->n_features, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows, idx,
                   B, 0.0f, grads, false, loss, nullptr, &a.batch);
    if (rc == ANTSRL_OK) rc = pop_train_tail(who, s, step, beta1, beta2, eps, running_loss, &a.adam, &t);
    if (rc != ANTSRL_OK) return rc;
    a.w1 = w1; a.b1 = b1; a.heads = heads; a.target_l3 = target_l3;
    a.adam.m = adam; a.adam.v = adam + LT_HEADS;
    const PopRunningLoss rl = {running_loss, first_loss != 0};
    return enqueued(antsrl_launch_pop_lintrain(a, t, s->n_members, rl, (hipStream_t)stream), who);
}

// ---- the population of explore agents (antsrl_popexplore.hip) -------------------------------------------------------------

// antsrl_pop_exptrain_sizes and antsrl_pop_jointtrain_sizes: a layer1-trained net's (antsrl_l1train.h), by its descriptor
template <class Net>
static int pop_l1t_sizes(const char *who, int32_t n_features, int64_t B, int32_t n_members, size_t *trained_floats,
                         size_t *workspace_stride, size_t *workspace_bytes, int32_t *launches)
{
    int rc = lt_features(who, n_features);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, Net::POP_MAX_B, POP_L1T_LIMIT);
    if (rc == ANTSRL_OK) rc = pop_n_members(who, n_members);
    if (rc != ANTSRL_OK) return rc;
    const size_t stride = l1t_pop_stride<Net>((int)B);
    if (trained_floats) *trained_floats = Net::floats(n_features);
    if (workspace_stride) *workspace_stride = stride;
    if (workspace_bytes) *workspace_bytes = stride * (size_t)n_members;
    if (launches) *launches = 2;
    return ANTSRL_OK;
}

// antsrl_pop_exptrain_step and antsrl_pop_jointtrain_step: the refusals in the training entries' order, then member 0's
// arguments (the slab's arrays, idx, grads, loss; the discount comes from the table; its partials are the front of the
// workspace, its dh behind them; the model, the target under the name its entry gives it, Adam's moments) and the launches
template <class Net>
static int pop_l1t_step(const char *who, const AntsPopSpec *s, float *model, const float *target, float *adam_m, float *adam_v,
                        const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                        const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                        const int64_t *idx, int64_t B, int64_t step, double beta1, double beta2, double eps, float *grads,
                        float *loss, double *running_loss, int first_loss, void *workspace, void *stream)
{
    PopTable t;
    L1TrainArgs a = {};
    int Em = 0;
    int rc = pop_spec(who, s, &t, &Em);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, Net::POP_MAX_B, POP_L1T_LIMIT);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(model, 4);
    if ((rc = require_named(who, Net::TARGET, target, 4)) != ANTSRL_OK) return rc;
    REQUIRE(adam_m, 4);
    REQUIRE(adam_v, 4);
    REQUIRE(idx, 8);
    REQUIRE(workspace, 256);
    rc = dqn_batch(who, s->n_features, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows, idx,
                   B, 0.0f, grads, false, loss, workspace, &a.batch);
    if (rc == ANTSRL_OK) rc = pop_train_tail(who, s, step, beta1, beta2, eps, running_loss, &a.adam, &t);
    if (rc != ANTSRL_OK) return rc;
    a.model = model; a.target = target;
    a.adam.m = adam_m; a.adam.v = adam_v;
    a.dh = (float *)((unsigned char *)workspace + l1t_dh_offset<Net>((int)B));
    a.blocks = l1t_blocks((int)B);
    const PopRunningLoss rl = {running_loss, first_loss != 0};
    return enqueued(Net::launch_pop(a, t, s->n_members, l1t_pop_stride<Net>((int)B), rl, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_explore_policy(const AntsPopSpec *s, const void *obs, const float *agent_state,
                                         const float *target_blocks, int8_t *rotation, void *stream)
{
    const char *who = "pop_explore_policy";
    int Em = 0;
    const int rc = pop_flat_policy(who, s, obs, agent_state, &Em);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(target_blocks, 4);
    REQUIRE(rotation, 1);
    PopExplorePolicyArgs a;
    a.obs = obs; a.agent_state = agent_state; a.target = target_blocks; a.rot = rotation;
    a.Mm = Em * s->n_ants; a.F = s->n_features; a.P = s->n_members;
    return enqueued(antsrl_launch_pop_explore_policy(a, s->obs_format == ANTSRL_OBS_BF16, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_exptrain_sizes(int32_t n_features, int64_t B, int32_t n_members, size_t *trained_floats,
                                         size_t *workspace_stride, size_t *workspace_bytes, int32_t *launches)
{
    return pop_l1t_sizes<ExpNet>("pop_exptrain_sizes", n_features, B, n_members, trained_floats, workspace_stride, workspace_bytes,
                                 launches);
}

extern "C" int antsrl_pop_exptrain_step(const AntsPopSpec *s, float *model, const float *target, float *adam_m, float *adam_v,
                                        const float *states, const float *agent_states, const int64_t *actions,
                                        const float *rewards, const float *new_states, const float *new_agent_states,
                                        const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, int64_t step,
                                        double beta1, double beta2, double eps, float *grads, float *loss,
                                        double *running_loss, int first_loss, void *workspace, void *stream)
{
    return pop_l1t_step<ExpNet>("pop_exptrain_step", s, model, target, adam_m, adam_v, states, agent_states, actions, rewards,
                                new_states, new_agent_states, dones, n_rows, idx, B, step, beta1, beta2, eps, grads, loss,
                                running_loss, first_loss, workspace, stream);
}

// ---- the population of joint agents (antsrl_popjoint.hip) ------------------------------------------------------------------

extern "C" int antsrl_pop_joint_policy(const AntsPopSpec *s, const void *obs, const float *agent_state,
                                       const float *model_blocks, const float *target_l3, int8_t *rotation,
                                       int8_t *pheromone, void *stream)
{
    const char *who = "pop_joint_policy";
    int Em = 0;
    const int rc = pop_flat_policy(who, s, obs, agent_state, &Em);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(model_blocks, 4);
    REQUIRE(target_l3, 4);
    REQUIRE(rotation, 1);
    REQUIRE(pheromone, 1);
    PopJointPolicyArgs a;
    a.obs = obs; a.agent_state = agent_state; a.model = model_blocks; a.target_l3 = target_l3;
    a.rot = rotation; a.ph = pheromone;
    a.Mm = Em * s->n_ants; a.F = s->n_features; a.P = s->n_members;
    return enqueued(antsrl_launch_pop_joint_policy(a, s->obs_format == ANTSRL_OBS_BF16, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_jointtrain_sizes(int32_t n_features, int64_t B, int32_t n_members, size_t *trained_floats,
                                           size_t *workspace_stride, size_t *workspace_bytes, int32_t *launches)
{
    return pop_l1t_sizes<JointNet>("pop_jointtrain_sizes", n_features, B, n_members, trained_floats, workspace_stride,
                                   workspace_bytes, launches);
}

extern "C" int antsrl_pop_jointtrain_step(const AntsPopSpec *s, float *model, const float *target_l3, float *adam_m,
                                          float *adam_v, const float *states, const float *agent_states, const int64_t *actions,
                                          const float *rewards, const float *new_states, const float *new_agent_states,
                                          const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, int64_t step,
                                          double beta1, double beta2, double eps, float *grads, float *loss,
                                          double *running_loss, int first_loss, void *workspace, void *stream)
{
    return pop_l1t_step<JointNet>("pop_jointtrain_step", s, model, target_l3, adam_m, adam_v, states, agent_states, actions,
                                  rewards, new_states, new_agent_states, dones, n_rows, idx, B, step, beta1, beta2, eps, grads,
                                  loss, running_loss, first_loss, workspace, stream);
}

// ---- the population of memory nets (antsrl_popmemtrain.hip) ----------------------------------------------------------------

// a spec and a shape (the memory net's or the rework net's) that have passed their own rules speak of the same rows
template <class Shape>
static int pop_same_features(const char *who, const AntsPopSpec *s, const Shape *shape)
{
    if (s->n_features == shape->n_features) return ANTSRL_OK;
    return fail(ANTSRL_E_INVALID, "%s: the spec's n_features = %d is not the shape's %d", who, s->n_features, shape->n_features);
}

// the shape's rules under the entry's name, then the two strides: the single trainer's state and workspace bytes, which
// must be multiples of 256 for every member's blocks to start as aligned as a single trainer's
static int pop_mem_layout(const char *who, const AntsMemNetShape *shape, int64_t B, MemNetDims *d, MemTrainLayout *L,
                          MemTrainWork *W)
{
    int rc = antsrl_memnet_dims(who, shape, d);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, MT_MAX_B);
    if (rc != ANTSRL_OK) return rc;
    antsrl_memtrain_state_layout(*d, L);
    antsrl_memtrain_work_layout(*d, (int)B, W);
    if (L->bytes % 256 || W->bytes % 256)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: a member's state of %zu bytes and workspace of %zu bytes must be multiples of 256",
                    who, L->bytes, W->bytes);
    return ANTSRL_OK;
}

extern "C" int antsrl_pop_memtrain_sizes(const AntsMemNetShape *shape, int64_t B, int32_t n_members, size_t *state_stride,
                                         size_t *trained_floats, size_t *work_stride, size_t *workspace_bytes,
                                         int32_t *launches)
{
    const char *who = "pop_memtrain_sizes";
    MemNetDims d;
    MemTrainLayout L;
    MemTrainWork W;
    int rc = pop_mem_layout(who, shape, B, &d, &L, &W);
    if (rc == ANTSRL_OK) rc = pop_n_members(who, n_members);
    if (rc != ANTSRL_OK) return rc;
    if (state_stride) *state_stride = L.bytes;
    if (trained_floats) *trained_floats = L.trained_floats;
    if (work_stride) *work_stride = W.bytes;
    if (workspace_bytes) *workspace_bytes = W.bytes * (size_t)n_members;
    if (launches) *launches = 17;
    return ANTSRL_OK;
}

// antsrl_dqn_minibatch's fields around the memory step's batch
struct PopMemBatch : MemTrainBatch {
    float *grads, *loss;
    long long n_rows;
    int B;
    float discount;
};

extern "C" int antsrl_pop_memtrain_step(const AntsPopSpec *s, const AntsMemNetShape *shape, void *net_states,
                                        const void *target_states, const float *states, const float *agent_states,
                                        const int64_t *actions, const float *rewards, const float *new_states,
                                        const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                                        const int64_t *idx, int64_t B, int64_t step, double beta1, double beta2, double eps,
                                        float *grads, float *loss, double *running_loss, int first_loss, void *workspace,
                                        void *stream)
{
    const char *who = "pop_memtrain_step";
    PopTable t;
    int Em = 0;
    MemNetDims d;
    MemTrainLayout L;
    MemTrainWork W;
    int rc = pop_spec(who, s, &t, &Em);
    if (rc == ANTSRL_OK) rc = pop_mem_layout(who, shape, B, &d, &L, &W);
    if (rc != ANTSRL_OK) return rc;
    if ((rc = pop_same_features(who, s, shape)) != ANTSRL_OK) return rc;
    REQUIRE(net_states, 256);
    REQUIRE(target_states, 256);
    REQUIRE(idx, 8);
    REQUIRE(workspace, 256);
    PopMemBatch bt = {};
    // member 0's minibatch: the slab's arrays, idx, grads, loss (the discount comes from the table)
    rc = antsrl_dqn_minibatch(who, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows, idx, B,
                              0.0f, grads, true, loss, &bt);
    AdamArgs adam = {};
    if (rc == ANTSRL_OK) rc = pop_train_tail(who, s, step, beta1, beta2, eps, running_loss, &adam, &t);
    if (rc != ANTSRL_OK) return rc;
    const PopRunningLoss rl = {running_loss, first_loss != 0};
    return enqueued(antsrl_launch_pop_memtrain(d, (unsigned char *)net_states, (const unsigned char *)target_states, bt, n_rows,
                                               (int)B, t, s->n_members, adam, grads, loss, rl, (unsigned char *)workspace,
                                               (hipStream_t)stream), who);
}

// ---- the memory agents' loop for a population (antsrl_popmemnet.hip; antsrl_population.hip's select and record) -------------

// the shape's rules under the entry's name, then a member's pack stride: the single net's packed bytes, which must be a
// multiple of 256 for every member's pack to start as aligned as a single net's (mn_layout rounds every block up to
// 256: checked here, not assumed)
static int pop_memnet_layout(const char *who, const AntsMemNetShape *shape, MemNetDims *d, size_t *pack_stride)
{
    const int rc = antsrl_memnet_dims(who, shape, d);
    if (rc != ANTSRL_OK) return rc;
    MemNetLayout L;
    antsrl_memnet_layout(*d, &L);
    if (L.bytes % 256)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: a member's pack of %zu bytes must be a multiple of 256", who, L.bytes);
    *pack_stride = L.bytes;
    return ANTSRL_OK;
}

// a population acts with the bf16 forward only (an unknown precision has been refused before this)
static int pop_memnet_bf16(const char *who, int precision)
{
    if (precision == ANTSRL_MEMNET_BF16) return ANTSRL_OK;
    return fail(ANTSRL_E_UNSUPPORTED, "%s: a population acts with bf16 operands only: precision ANTSRL_MEMNET_FP32 is not built", who);
}

// what the loop's entries check of (spec, shape) together: both sets of rules, then that they speak of the same rows
static int pop_mem_spec(const char *who, const AntsPopSpec *s, const AntsMemNetShape *shape, PopTable *t, int *Em, MemNetDims *d,
                        size_t *pack_stride)
{
    int rc = pop_spec(who, s, t, Em);
    if (rc == ANTSRL_OK) rc = pop_memnet_layout(who, shape, d, pack_stride);
    if (rc != ANTSRL_OK) return rc;
    return pop_same_features(who, s, shape);
}

extern "C" int antsrl_pop_memnet_sizes(const AntsMemNetShape *shape, int precision, int32_t n_members, size_t *pack_stride,
                                       size_t *packed_bytes)
{
    const char *who = "pop_memnet_sizes";
    MemNetDims d;
    size_t stride = 0;
    int rc = antsrl_memnet_precision(who, precision);
    if (rc == ANTSRL_OK) rc = pop_memnet_layout(who, shape, &d, &stride);
    if (rc == ANTSRL_OK) rc = pop_memnet_bf16(who, precision);
    if (rc == ANTSRL_OK) rc = pop_n_members(who, n_members);
    if (rc != ANTSRL_OK) return rc;
    if (pack_stride) *pack_stride = stride;
    if (packed_bytes) *packed_bytes = stride * (size_t)n_members;
    return ANTSRL_OK;
}

extern "C" int antsrl_pop_policy_memory(const AntsPopSpec *s, const AntsMemNetShape *shape, int precision, const void *packed,
                                        const void *obs, const float *agent_state, const float *mem_in, float *mem_out,
                                        int8_t *rotation, int8_t *pheromone, float *q_out, void *stream)
{
    const char *who = "pop_policy_memory";
    PopTable t;
    int Em = 0;
    MemNetDims d;
    size_t stride = 0;
    int rc = antsrl_memnet_precision(who, precision);
    if (rc == ANTSRL_OK) rc = pop_mem_spec(who, s, shape, &t, &Em, &d, &stride);
    if (rc == ANTSRL_OK) rc = pop_memnet_bf16(who, precision);
    if (rc != ANTSRL_OK) return rc;
    const long long Mm = (long long)Em * s->n_ants;
    if (Mm > 0x7fffffffLL - 32 * 4) // (a workgroup has at most four waves of 32 ants: the launcher rounds Mm up to that)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: n_envs / n_members * n_ants = %lld: the tile count of a member's grid row must fit "
                                          "an int (at most 2^31 - 1 - 128 ants per member)", who, Mm);
    const bool bf16 = s->obs_format == ANTSRL_OBS_BF16;
    REQUIRE(packed, 256);
    REQUIRE(obs, bf16 ? 2 : 4);
    REQUIRE(agent_state, 4);
    REQUIRE(mem_in, 4);
    REQUIRE(mem_out, 4);
    REQUIRE(rotation, 1);
    if ((uintptr_t)q_out & 3) return fail(ANTSRL_E_INVALID, "%s: q_out must be 4-byte aligned", who);
    return enqueued(antsrl_launch_pop_memnet((const unsigned char *)packed, stride, d, obs, bf16, agent_state, mem_in, (int)Mm,
                                             s->n_members, mem_out, rotation, pheromone, q_out, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_memory_select(const AntsPopSpec *s, const AntsMemNetShape *shape, uint64_t step, int8_t *rotation,
                                        int8_t *pheromone, const float *mem_old, float *mem_next, uint8_t *explored,
                                        void *stream)
{
    const char *who = "pop_memory_select";
    PopTable t;
    int Em = 0;
    MemNetDims d;
    size_t stride = 0;
    const int rc = pop_mem_spec(who, s, shape, &t, &Em, &d, &stride);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(rotation, 1);
    REQUIRE(pheromone, 1);
    REQUIRE(mem_old, 4);
    REQUIRE(mem_next, 4);
    if (mem_old != mem_next) { // the same buffer, or two that do not touch (antsrl_agent_select's rule, on the whole batch)
        const uintptr_t o = (uintptr_t)mem_old, n = (uintptr_t)mem_next;
        const uintptr_t bytes = (uintptr_t)s->n_envs * (uintptr_t)s->n_ants * (uintptr_t)d.mem * 4;
        if (o < n + bytes && n < o + bytes) return fail(ANTSRL_E_INVALID, "%s: mem_old and mem_next overlap without being equal", who);
    }
    SelArgs a; // member 0's Em environments; seed and epsilon come from the table
    antsrl_sel_args(0, step, s->env_id_base, Em, s->n_ants, 0.0, d.n_rot, d.n_ph, &a);
    a.rot = rotation; a.ph = pheromone; a.mem_old = mem_old; a.mem_next = mem_next; a.explored = explored;
    // antsrl_agent_select's rule for float4 elements, which then holds for every member's offset as well: a member's
    // halves start Em * env_floats floats behind the previous member's, a multiple of 4 floats = 16 bytes
    const uint64_t env_floats = (uint64_t)s->n_ants * (uint64_t)d.mem; // < 2^36
    const bool vec = env_floats % 4 == 0 && (((uintptr_t)mem_old | (uintptr_t)mem_next) & 15) == 0;
    const uint64_t env_elems = vec ? env_floats / 4 : env_floats;
    if (env_elems > 0xffffffffULL)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: n_ants * mem_size = %llu is too large", who, (unsigned long long)env_floats);
    a.env_elems = (uint32_t)env_elems;
    a.mem_elems = env_elems * (uint64_t)Em; // member 0's
    return enqueued(antsrl_launch_pop_memory_select(a, t, s->n_members, Em, vec, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_memory_record_pre(const AntsPopSpec *s, const AntsMemNetShape *shape, uint64_t step, int64_t K,
                                            int64_t head, int64_t max_len, const void *obs, const float *agent_state,
                                            const float *memory, const int8_t *rotation, const int8_t *pheromone,
                                            float *states, float *agent_states, int64_t *actions, void *stream)
{
    return pop_record_pre("pop_memory_record_pre", s, true, shape, step, K, head, max_len, obs, agent_state, memory, rotation,
                          pheromone, states, agent_states, actions, stream);
}

extern "C" int antsrl_pop_memory_record_post(const AntsPopSpec *s, const AntsMemNetShape *shape, uint64_t step, int64_t K,
                                             int64_t head, int64_t max_len, const void *obs, const float *agent_state,
                                             const float *memory, const float *reward, const uint8_t *done, float *rewards,
                                             float *new_states, float *new_agent_states, uint8_t *dones, void *stream)
{
    return pop_record_post("pop_memory_record_post", s, true, shape, step, K, head, max_len, obs, agent_state, memory, reward, done,
                           rewards, new_states, new_agent_states, dones, stream);
}

// ---- the population of rework agents (antsrl_poprework.hip) ----------------------------------------------------------------

// the floats of a member's collapsed buffer
static size_t pop_rw_collapsed_floats(const ReworkDims &d) { return (size_t)(d.n_rot + d.n_ph) * (size_t)(d.D + 1); }

// what the two acting entries check: the spec's rules, the shape's (antsrl_reworkapi.hip's), that they speak of the same
// rows, the slice rule, then the pointers; fills member 0's arguments
static int pop_rw_policy(const char *who, const AntsPopSpec *s, const AntsReworkShape *shape, const void *collapsed, const void *obs,
                         const float *agent_state, int8_t *rotation, int8_t *pheromone, float *q_out, PopTable *t,
                         PopReworkActArgs *a)
{
    int Em = 0;
    int rc = pop_spec(who, s, t, &Em);
    if (rc == ANTSRL_OK) rc = rework_check(shape, &a->d, who);
    if (rc == ANTSRL_OK) rc = pop_same_features(who, s, shape);
    if (rc == ANTSRL_OK) rc = pop_slice_rule(who, s, Em);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(collapsed, 4);
    REQUIRE(obs, 16);
    REQUIRE(agent_state, 4);
    REQUIRE(rotation, 1);
    REQUIRE(pheromone, 1);
    if ((uintptr_t)q_out & 3) return fail(ANTSRL_E_INVALID, "%s: q_out must be 4-byte aligned", who);
    a->collapsed = (const float *)collapsed; a->obs = obs; a->agent_state = agent_state;
    a->rot = rotation; a->ph = pheromone; a->q_out = q_out;
    a->Mm = Em * s->n_ants; a->Em = Em; a->P = s->n_members;
    return ANTSRL_OK;
}

extern "C" int antsrl_pop_rework_collapse(const AntsReworkShape *shape, int32_t n_members, const float *target_blocks,
                                          float *collapsed, void *stream)
{
    const char *who = "pop_rework_collapse";
    PopReworkCollapseArgs a = {};
    int rc = rework_check(shape, &a.d, who);
    if (rc == ANTSRL_OK) rc = pop_n_members(who, n_members);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(target_blocks, 4);
    REQUIRE(collapsed, 4);
    ReworkTrainLayout L;
    antsrl_reworktrain_layout(a.d, 1, &L);
    for (int i = 0; i <= 2 * RW_LAYERS; ++i) a.off[i] = L.off[i];
    a.blocks = target_blocks; a.collapsed = collapsed;
    return enqueued(antsrl_launch_pop_rework_collapse(a, n_members, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_policy_rework(const AntsPopSpec *s, const AntsReworkShape *shape, const void *collapsed,
                                        const void *obs, const float *agent_state, int8_t *rotation, int8_t *pheromone,
                                        float *q_out, void *stream)
{
    const char *who = "pop_policy_rework";
    PopTable t;
    PopReworkActArgs a = {};
    const int rc = pop_rw_policy(who, s, shape, collapsed, obs, agent_state, rotation, pheromone, q_out, &t, &a);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(antsrl_launch_pop_rework_act(a, t, s->obs_format == ANTSRL_OBS_BF16, false, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_policy_rework_select(const AntsPopSpec *s, const AntsReworkShape *shape, const void *collapsed,
                                               const void *obs, const float *agent_state, uint64_t step, int8_t *rotation,
                                               int8_t *pheromone, uint8_t *explored, float *q_out, void *stream)
{
    const char *who = "pop_policy_rework_select";
    PopTable t;
    PopReworkActArgs a = {};
    const int rc = pop_rw_policy(who, s, shape, collapsed, obs, agent_state, rotation, pheromone, q_out, &t, &a);
    if (rc != ANTSRL_OK) return rc;
    // member 0's select; seed and epsilon come from the table
    a.sel.step = step; a.sel.explored = explored;
    a.sel.env_base = (uint32_t)s->env_id_base; a.sel.n_ants = (uint32_t)s->n_ants;
    return enqueued(antsrl_launch_pop_rework_act(a, t, s->obs_format == ANTSRL_OBS_BF16, true, (hipStream_t)stream), who);
}

extern "C" int antsrl_pop_reworktrain_sizes(const AntsReworkShape *shape, int64_t B, int32_t n_members, size_t *trained_floats,
                                            size_t *collapsed_floats, size_t *workspace_stride, size_t *workspace_bytes,
                                            int32_t *launches)
{
    const char *who = "pop_reworktrain_sizes";
    ReworkDims d;
    int rc = rework_check(shape, &d, who);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, RT_MAX_B);
    if (rc == ANTSRL_OK) rc = pop_n_members(who, n_members);
    if (rc != ANTSRL_OK) return rc;
    ReworkTrainLayout L;
    antsrl_reworktrain_layout(d, (int)B, &L);
    const size_t stride = (L.bytes + 255) / 256 * 256; // (the layout rounds every part up to 256: the stride is L.bytes)
    if (trained_floats) *trained_floats = L.off[2 * RW_LAYERS];
    if (collapsed_floats) *collapsed_floats = pop_rw_collapsed_floats(d);
    if (workspace_stride) *workspace_stride = stride;
    if (workspace_bytes) *workspace_bytes = stride * (size_t)n_members;
    if (launches) *launches = 4;
    return ANTSRL_OK;
}

extern "C" int antsrl_pop_reworktrain_step(const AntsPopSpec *s, const AntsReworkShape *shape, float *model,
                                           const float *target_collapsed, float *adam_m, float *adam_v, const float *states,
                                           const float *agent_states, const int64_t *actions, const float *rewards,
                                           const float *new_states, const float *new_agent_states, const uint8_t *dones,
                                           int64_t n_rows, const int64_t *idx, int64_t B, int64_t step, double beta1,
                                           double beta2, double eps, float *grads, float *loss, double *running_loss,
                                           int first_loss, void *workspace, void *stream)
{
    const char *who = "pop_reworktrain_step";
    PopTable t;
    ReworkTrainArgs a = {};
    int Em = 0;
    int rc = pop_spec(who, s, &t, &Em);
    if (rc == ANTSRL_OK) rc = rework_check(shape, &a.d, who);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, RT_MAX_B);
    if (rc == ANTSRL_OK) rc = pop_same_features(who, s, shape);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(model, 4);
    REQUIRE(target_collapsed, 4);
    REQUIRE(adam_m, 4);
    REQUIRE(adam_v, 4);
    REQUIRE(idx, 8);
    REQUIRE(workspace, 256);
    // member 0's minibatch: the slab's arrays, idx, grads, loss (the discount comes from the table)
    rc = antsrl_dqn_minibatch(who, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows, idx, B,
                              0.0f, grads, false, loss, &a);
    if (rc == ANTSRL_OK) rc = pop_train_tail(who, s, step, beta1, beta2, eps, running_loss, &a.adam, &t);
    if (rc != ANTSRL_OK) return rc;
    antsrl_reworktrain_layout(a.d, (int)B, &a.L); // the single step's for this B: `parts` with it
    a.work = (unsigned char *)workspace;
    a.dq_rot = (float)(2.0 / ((double)a.d.n_rot * (double)B));
    a.dq_ph = (float)(2.0 / ((double)a.d.n_ph * (double)B));
    a.loss_rot = (float)(1.0 / ((double)a.d.n_rot * (double)B));
    a.loss_ph = (float)(1.0 / ((double)a.d.n_ph * (double)B));
    a.model = model; a.target = target_collapsed;
    a.adam.m = adam_m; a.adam.v = adam_v;
    const PopRunningLoss rl = {running_loss, first_loss != 0};
    return enqueued(antsrl_launch_pop_reworktrain(a, t, s->n_members, (a.L.bytes + 255) / 256 * 256, rl, (hipStream_t)stream), who);
}

// ---- population-based training (antsrl_popfitness.hip, antsrl_checkpoint.hip) -----------------------------------------------

extern "C" int antsrl_pop_fitness(const double *episode_reward, int n_envs, int n_ants, int n_members, double *row, void *stream)
{
    const char *who = "pop_fitness";
    REQUIRE(episode_reward, 8);
    REQUIRE(row, 8);
    int rc = pop_n_members(who, n_members);
    if (rc != ANTSRL_OK) return rc;
    if (n_envs < 1 || n_ants < 1) return fail(ANTSRL_E_INVALID, "%s: n_envs and n_ants must be >= 1 (%d, %d)", who, n_envs, n_ants);
    if (n_envs % n_members)
        return fail(ANTSRL_E_INVALID, "%s: n_envs = %d is not a multiple of n_members = %d (members own equal shares)", who, n_envs,
                    n_members);
    const uintptr_t e0 = (uintptr_t)episode_reward, e1 = e0 + (uintptr_t)n_envs * (uintptr_t)n_ants * 8;
    const uintptr_t r0 = (uintptr_t)row, r1 = r0 + (uintptr_t)n_members * 24;
    if (r0 < e1 && e0 < r1) return fail(ANTSRL_E_INVALID, "%s: row overlaps episode_reward", who);
    return enqueued(antsrl_launch_pop_fitness(episode_reward, n_envs / n_members, n_ants, n_members, row, (hipStream_t)stream), who);
}

// Every pair and every per-member array in ONE launch of k_env_copy: the fork's table (antsrl_checkpoint.h) with the
// members as its rows and src == dst == base[a].  The kernel takes 16 bytes per lane where a pair's two rows are
// congruent modulo 16, 4 bytes where modulo 4 only (a block of 9603 floats), single bytes otherwise, and touches no byte
// outside a row.
extern "C" int antsrl_pop_exploit(int n_arrays, void *const *base, const uint64_t *row_bytes, int n_members, int n_pairs,
                                  const int32_t *src, const int32_t *dst, void *stream)
{
    const char *who = "pop_exploit";
    if (n_arrays < 1 || n_arrays > ENV_COPY_MAX_ARRAYS)
        return fail(ANTSRL_E_INVALID, "%s: n_arrays must be in [1, ENV_COPY_MAX_ARRAYS = %d] (%d)", who, ENV_COPY_MAX_ARRAYS, n_arrays);
    if (n_pairs < 0 || n_pairs > ENV_COPY_MAX_PAIRS)
        return fail(ANTSRL_E_INVALID, "%s: n_pairs must be in [0, ENV_COPY_MAX_PAIRS = %d] (%d)", who, ENV_COPY_MAX_PAIRS, n_pairs);
    int rc = pop_n_members(who, n_members);
    if (rc != ANTSRL_OK) return rc;
    if (!base || !row_bytes) return fail(ANTSRL_E_INVALID, "%s: NULL base or row_bytes", who);
    EnvCopyTable t;
    memset(&t, 0, sizeof(t));
    uint64_t chunks = 0;
    for (int a = 0; a < n_arrays; ++a) {
        if (row_bytes[a] == 0) return fail(ANTSRL_E_INVALID, "%s: row_bytes[%d] is 0", who, a);
        if (!base[a]) return fail(ANTSRL_E_INVALID, "%s: base[%d] is NULL", who, a);
        EnvCopyArray &e = t.a[a];
        e.src = e.dst = (unsigned char *)base[a];
        e.bytes = row_bytes[a];
        e.first_chunk = (uint32_t)chunks;
        chunks += env_copy_chunks(e.bytes);
        if (chunks > 0x7fffffffull) return fail(ANTSRL_E_UNSUPPORTED, "%s: the rows are too large for one copy", who);
    }
    if (n_pairs == 0) return ANTSRL_OK; // nothing to copy: no launch
    if (!src || !dst) return fail(ANTSRL_E_INVALID, "%s: NULL src or dst", who);
    static_assert(ANTSRL_POP_MAX <= 64, "a member set is one 64-bit word");
    uint64_t is_dst = 0;
    for (int i = 0; i < n_pairs; ++i) { // (stops at the first repeated dst: at most n_members + 1 entries are read)
        if (src[i] < 0 || src[i] >= n_members) return fail(ANTSRL_E_INVALID, "%s: src[%d] = %d is not in [0, %d)", who, i, src[i], n_members);
        if (dst[i] < 0 || dst[i] >= n_members) return fail(ANTSRL_E_INVALID, "%s: dst[%d] = %d is not in [0, %d)", who, i, dst[i], n_members);
        if (is_dst >> dst[i] & 1u) return fail(ANTSRL_E_INVALID, "%s: dst %d appears twice (dst[%d])", who, dst[i], i);
        is_dst |= 1ull << dst[i];
    }
    for (int i = 0; i < n_pairs; ++i)
        if (is_dst >> src[i] & 1u) return fail(ANTSRL_E_INVALID, "%s: member %d is a src (src[%d]) and a dst", who, src[i], i);
    t.n_arrays = n_arrays;
    t.rows = n_pairs;
    t.chunks_per_row = (uint32_t)chunks;
    for (int i = 0; i < n_pairs; ++i) {
        t.pair_src[i] = (uint16_t)src[i];
        t.pair_dst[i] = (uint16_t)dst[i];
    }
    return enqueued(antsrl_launch_env_copy(t, (hipStream_t)stream), who);
}
