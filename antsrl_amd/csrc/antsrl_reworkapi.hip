// antsrl_reworkapi.hip — the rework agent's part of the C-ABI of libantsrl_hip.so (include/antsrl.h, "The rework agent's
// net"): antsrl_rework_collapsed_bytes, antsrl_rework_collapse and antsrl_policy_rework in front of antsrl_rework.hip's
// kernels (antsrl_policy_rework_select: the forward pass and the epsilon-greedy select in one), and behind them its training step ("The rework agent's training step"): antsrl_reworktrain_sizes / _grad /
// _apply / _step in front of antsrl_reworktrain.hip's four, with the argument rules of the linear and explore agents'
// (antsrl_linapi.hip): the minibatch's are antsrl_dqn_minibatch's (antsrl_dqn.h) for all three.
//
// Host-side only: validates every argument before any HIP call and enqueues on the caller's stream.  No handle, no
// allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_device.h"
#include "antsrl_dqn.h" // antsrl_dqn_B, antsrl_dqn_minibatch
#include "antsrl_fail.h"
#include "antsrl_loopapi.h" // antsrl_check_batch, antsrl_check_epsilon, antsrl_check_obs_format
#include "antsrl_rework.h"
#include "antsrl_reworkapi.h" // rework_check
#include "antsrl_reworktrain.h"

extern "C" int antsrl_rework_collapsed_bytes(const AntsReworkShape *s, size_t *bytes)
{
    const char *who = "rework_collapsed_bytes";
    ReworkDims d;
    const int rc = rework_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!bytes) return fail(ANTSRL_E_INVALID, "%s: NULL bytes", who);
    *bytes = sizeof(float) * ((size_t)(d.n_rot + d.n_ph) * d.D + (size_t)(d.n_rot + d.n_ph));
    return ANTSRL_OK;
}

extern "C" int antsrl_rework_collapse(const AntsReworkShape *s, const float *const *params, void *collapsed, void *stream)
{
    const char *who = "rework_collapse";
    ReworkDims d;
    const int rc = rework_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!params || !collapsed) return fail(ANTSRL_E_INVALID, "%s: params and collapsed are required", who);
    if ((uintptr_t)collapsed & 3) return fail(ANTSRL_E_INVALID, "%s: collapsed must be 4-byte aligned", who);
    ReworkParams P;
    for (int i = 0; i < 2 * RW_LAYERS; ++i) {
        if (!params[i]) return fail(ANTSRL_E_INVALID, "%s: params[%d] is NULL", who, i);
        if ((uintptr_t)params[i] & 3) return fail(ANTSRL_E_INVALID, "%s: params[%d] must be 4-byte aligned", who, i);
        P.p[i] = params[i];
    }
    return enqueued(antsrl_launch_rework_collapse(P, d, (float *)collapsed, (hipStream_t)stream), who);
}

// the shape and the operands of a forward pass, with or without the select behind it
static int rework_act_check(const char *who, const AntsReworkShape *s, ReworkDims *d, const void *collapsed, const void *obs,
                            int obs_format, const float *agent_state, const int8_t *rotation, const int8_t *pheromone,
                            const float *q_out)
{
    const int rc = rework_check(s, d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!collapsed || !obs || !agent_state || !rotation || !pheromone)
        return fail(ANTSRL_E_INVALID, "%s: collapsed, obs, agent_state, rotation, pheromone are required", who);
    if (((uintptr_t)collapsed | (uintptr_t)obs | (uintptr_t)agent_state | (uintptr_t)q_out) & 3)
        return fail(ANTSRL_E_INVALID, "%s: collapsed, obs, agent_state and q_out must be 4-byte aligned", who);
    return antsrl_check_obs_format(who, obs_format);
}

extern "C" int antsrl_policy_rework(const AntsReworkShape *s, const void *collapsed, const void *obs, int obs_format,
                                    const float *agent_state, int64_t n_ants, int8_t *rotation, int8_t *pheromone,
                                    float *q_out, void *stream)
{
    const char *who = "policy_rework";
    ReworkDims d;
    const int rc = rework_act_check(who, s, &d, collapsed, obs, obs_format, agent_state, rotation, pheromone, q_out);
    if (rc != ANTSRL_OK) return rc;
    if (n_ants < 0 || n_ants > 0x7fffffff) return fail(ANTSRL_E_INVALID, "%s: n_ants must be in [0, 2^31)", who);
    if (n_ants == 0) return ANTSRL_OK; // nothing to do, nothing launched
    return enqueued(antsrl_launch_rework_act((const float *)collapsed, d, obs, obs_format == ANTSRL_OBS_BF16, agent_state,
                                             (int)n_ants, rotation, pheromone, q_out, (hipStream_t)stream),
                    who);
}

extern "C" int antsrl_policy_rework_select(const AntsReworkShape *s, const void *collapsed, const void *obs, int obs_format,
                                           const float *agent_state, uint64_t seed, uint64_t step, int32_t env_id_base,
                                           int32_t n_envs, int32_t n_ants, double epsilon, int8_t *rotation,
                                           int8_t *pheromone, uint8_t *explored, float *q_out, void *stream)
{
    const char *who = "policy_rework_select";
    ReworkDims d;
    int rc = rework_act_check(who, s, &d, collapsed, obs, obs_format, agent_state, rotation, pheromone, q_out);
    if (rc != ANTSRL_OK) return rc;
    if ((rc = antsrl_check_batch(who, env_id_base, n_envs, n_ants)) != ANTSRL_OK) return rc;
    if ((rc = antsrl_check_epsilon(who, -1, epsilon)) != ANTSRL_OK) return rc;
    ReworkSelect sel = {};
    sel.seed = seed; sel.step = step; sel.epsilon = epsilon; sel.explored = explored;
    sel.env_base = (uint32_t)env_id_base; sel.n_ants = (uint32_t)n_ants;
    return enqueued(antsrl_launch_rework_act_select((const float *)collapsed, d, obs, obs_format == ANTSRL_OBS_BF16, agent_state,
                                                    n_envs * n_ants, sel, rotation, pheromone, q_out, (hipStream_t)stream),
                    who);
}

// ---- the training step (antsrl_reworktrain.hip) ----------------------------------------------------------------------------

extern "C" int antsrl_reworktrain_sizes(const AntsReworkShape *s, int64_t B, size_t *params_floats, size_t *workspace_bytes,
                                        int32_t *launches)
{
    const char *who = "reworktrain_sizes";
    ReworkDims d;
    int rc = rework_check(s, &d, who);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, RT_MAX_B);
    if (rc != ANTSRL_OK) return rc;
    ReworkTrainLayout L;
    antsrl_reworktrain_layout(d, (int)B, &L);
    if (params_floats) *params_floats = L.off[2 * RW_LAYERS];
    if (workspace_bytes) *workspace_bytes = L.bytes;
    if (launches) *launches = 4;
    return ANTSRL_OK;
}

// the shape, the nets, the workspace and (antsrl_dqn_minibatch) the minibatch of the gradient stage and the fused step
static int rt_args(const char *who, const AntsReworkShape *s, float *model, const float *target_collapsed,
                   const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                   const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                   const int64_t *idx, int64_t B, float discount, float *grads, bool grads_required, float *loss,
                   void *workspace, ReworkTrainArgs *a)
{
    int rc = rework_check(s, &a->d, who);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, RT_MAX_B);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(model, 4);
    REQUIRE(target_collapsed, 4);
    REQUIRE(workspace, 256);
    if ((rc = antsrl_dqn_minibatch(who, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows,
                                   idx, B, discount, grads, grads_required, loss, a)) != ANTSRL_OK)
        return rc;
    antsrl_reworktrain_layout(a->d, (int)B, &a->L);
    a->work = (unsigned char *)workspace;
    a->dq_rot = (float)(2.0 / ((double)a->d.n_rot * (double)B));
    a->dq_ph = (float)(2.0 / ((double)a->d.n_ph * (double)B));
    a->loss_rot = (float)(1.0 / ((double)a->d.n_rot * (double)B));
    a->loss_ph = (float)(1.0 / ((double)a->d.n_ph * (double)B));
    a->model = model; a->target = target_collapsed;
    return ANTSRL_OK;
}

extern "C" int antsrl_reworktrain_grad(const AntsReworkShape *s, const float *model, const float *target_collapsed,
                                       const float *states, const float *agent_states, const int64_t *actions,
                                       const float *rewards, const float *new_states, const float *new_agent_states,
                                       const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, float discount,
                                       float *grads, float *loss, void *workspace, void *stream)
{
    const char *who = "reworktrain_grad";
    ReworkTrainArgs a = {};
    const int rc = rt_args(who, s, const_cast<float *>(model), target_collapsed, states, agent_states, actions, rewards,
                           new_states, new_agent_states, dones, n_rows, idx, B, discount, grads, true, loss, workspace, &a);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(antsrl_launch_reworktrain(a, (hipStream_t)stream), who); // a.adam.on == 0: model is only read
}

extern "C" int antsrl_reworktrain_apply(const AntsReworkShape *s, float *model, float *adam_m, float *adam_v,
                                        const float *grads, int64_t step, double lr, double beta1, double beta2, double eps,
                                        void *stream)
{
    const char *who = "reworktrain_apply";
    ReworkDims d;
    const int rc = rework_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(model, 4);
    ReworkTrainLayout L;
    antsrl_reworktrain_layout(d, 1, &L);
    return antsrl_adam_apply(who, model, adam_m, adam_v, grads, step, lr, beta1, beta2, eps, (int)L.off[2 * RW_LAYERS], stream);
}

extern "C" int antsrl_reworktrain_step(const AntsReworkShape *s, float *model, const float *target_collapsed, float *adam_m,
                                       float *adam_v, const float *states, const float *agent_states, const int64_t *actions,
                                       const float *rewards, const float *new_states, const float *new_agent_states,
                                       const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, float discount,
                                       int64_t step, double lr, double beta1, double beta2, double eps, float *grads,
                                       float *loss, void *workspace, void *stream)
{
    const char *who = "reworktrain_step";
    ReworkTrainArgs a = {};
    int rc = rt_args(who, s, model, target_collapsed, states, agent_states, actions, rewards, new_states, new_agent_states,
                     dones, n_rows, idx, B, discount, grads, false, loss, workspace, &a);
    if (rc == ANTSRL_OK) rc = antsrl_adam_step(who, adam_m, adam_v, step, lr, beta1, beta2, eps, &a.adam);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(antsrl_launch_reworktrain(a, (hipStream_t)stream), who);
}
