// antsrl_linapi.hip — the linear agent's training step in the C-ABI of libantsrl_hip.so (include/antsrl.h, "The linear
// agent's training step"): antsrl_lintrain_sizes / _grad / _apply / _step in front of antsrl_lintrain.hip's kernels, and
// behind them the explore agent's ("The explore agent's training step"): antsrl_exptrain_sizes / _grad / _apply / _step
// in front of antsrl_exptrain.hip's, and the joint step's ("The joint training step"): antsrl_jointtrain_sizes / _grad /
// _apply / _step in front of antsrl_jointtrain.hip's, all with the same argument rules; the last two nets' entries are
// calls of one body per stage over the net's descriptor (antsrl_l1train.h).  antsrl_dqn_minibatch (antsrl_dqn.h) checks and fills
// what every step takes from the replay arrays, the rework agent's (antsrl_reworkapi.hip) included; dqn_batch adds what
// the 32-wide nets keep in DqnBatch, antsrl_adam_step (antsrl_adam.h) Adam's part; an entry checks its own net's
// pointers, its limit on B and its workspace rule.
//
// Host-side only: validates every argument before any HIP call and enqueues on the caller's stream.  No handle, no
// allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_adam.h"
#include "antsrl_device.h"
#include "antsrl_dqn.h"
#include "antsrl_exptrain.h"
#include "antsrl_fail.h"
#include "antsrl_jointtrain.h"
#include "antsrl_lintrain.h"

#define LT_MAX_B (1 << 24)

int lt_features(const char *who, int32_t n_features)
{
    if (n_features < 1) return fail(ANTSRL_E_INVALID, "%s: n_features must be >= 1 (%d)", who, n_features);
    if (n_features + 2 > 1024) return fail(ANTSRL_E_UNSUPPORTED, "%s: n_features + 2 = %d > 1024", who, n_features + 2);
    return ANTSRL_OK;
}

static int lt_B(const char *who, int64_t B)
{
    if (B < 1 || B > LT_MAX_B) return fail(ANTSRL_E_INVALID, "%s: B must be in [1, 2^24] (%lld)", who, (long long)B);
    return ANTSRL_OK;
}

// the minibatch of a gradient stage or a fused step, for n_features and B its entry has checked: antsrl_dqn_minibatch's
// part, then what the 32-wide nets add; workspace (checked by the entry's own rule; NULL for a step of one workgroup
// per net, the population's) becomes the partials.  Declared in antsrl_dqn.h.
int dqn_batch(const char *who, int32_t n_features, const float *states, const float *agent_states, const int64_t *actions,
              const float *rewards, const float *new_states, const float *new_agent_states, const uint8_t *dones,
              int64_t n_rows, const int64_t *idx, int64_t B, float discount, float *grads, bool grads_required, float *loss,
              void *workspace, DqnBatch *q)
{
    const int rc = antsrl_dqn_minibatch(who, states, agent_states, actions, rewards, new_states, new_agent_states, dones,
                                        n_rows, idx, B, discount, grads, grads_required, loss, q);
    if (rc != ANTSRL_OK) return rc;
    q->partials = (float *)workspace;
    q->F = n_features; q->ksteps = (n_features + 15) / 16; q->ntiles = ((int)B + 31) / 32;
    q->dq_scale = (float)(2.0 / (3.0 * (double)B));
    q->loss_scale = (float)(1.0 / (3.0 * (double)B));
    return ANTSRL_OK;
}

// ---- the linear agent's training step (antsrl_lintrain.hip) ---------------------------------------------------------------

extern "C" int antsrl_lintrain_sizes(int32_t n_features, int64_t B, size_t *trained_floats, size_t *workspace_bytes,
                                     int32_t *launches)
{
    const char *who = "lintrain_sizes";
    int rc = lt_features(who, n_features);
    if (rc == ANTSRL_OK) rc = lt_B(who, B);
    if (rc != ANTSRL_OK) return rc;
    const int blocks = antsrl_lintrain_blocks((int)B, n_features);
    if (trained_floats) *trained_floats = LT_HEADS;
    if (workspace_bytes) *workspace_bytes = (size_t)blocks * LT_PART * sizeof(float);
    if (launches) *launches = blocks == 1 ? 1 : 2;
    return ANTSRL_OK;
}

// the net and the workspace of the gradient stage and the fused step
static int lt_net(const char *who, int32_t n_features, int64_t B, const float *w1, const float *b1, float *heads,
                  const float *target_l3, void *workspace, LinTrainArgs *a)
{
    int rc = lt_features(who, n_features);
    if (rc == ANTSRL_OK) rc = lt_B(who, B);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(w1, 4);
    REQUIRE(b1, 4);
    REQUIRE(heads, 4);
    REQUIRE(target_l3, 4);
    if (antsrl_lintrain_blocks((int)B, n_features) > 1) REQUIRE(workspace, 256);
    a->w1 = w1; a->b1 = b1; a->heads = heads; a->target_l3 = target_l3;
    return ANTSRL_OK;
}

extern "C" int antsrl_lintrain_grad(int32_t n_features, const float *w1, const float *b1, const float *heads,
                                    const float *target_l3, const float *states, const float *agent_states,
                                    const int64_t *actions, const float *rewards, const float *new_states,
                                    const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx,
                                    int64_t B, float discount, float *grads, float *loss, void *workspace, void *stream)
{
    const char *who = "lintrain_grad";
    LinTrainArgs a = {};
    int rc = lt_net(who, n_features, B, w1, b1, const_cast<float *>(heads), target_l3, workspace, &a);
    if (rc == ANTSRL_OK)
        rc = dqn_batch(who, n_features, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows,
                       idx, B, discount, grads, true, loss, workspace, &a.batch);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(antsrl_launch_lintrain(a, (hipStream_t)stream), who); // a.adam.on == 0: heads is only read
}

extern "C" int antsrl_lintrain_apply(float *heads, float *adam_m, float *adam_v, const float *grads, int64_t step, double lr,
                                     double beta1, double beta2, double eps, void *stream)
{
    const char *who = "lintrain_apply";
    REQUIRE(heads, 4);
    return antsrl_adam_apply(who, heads, adam_m, adam_v, grads, step, lr, beta1, beta2, eps, LT_HEADS, stream);
}

extern "C" int antsrl_lintrain_step(int32_t n_features, const float *w1, const float *b1, float *heads,
                                    const float *target_l3, float *adam_m, float *adam_v, const float *states,
                                    const float *agent_states, const int64_t *actions, const float *rewards,
                                    const float *new_states, const float *new_agent_states, const uint8_t *dones,
                                    int64_t n_rows, const int64_t *idx, int64_t B, float discount, int64_t step, double lr,
                                    double beta1, double beta2, double eps, float *grads, float *loss, void *workspace,
                                    void *stream)
{
    const char *who = "lintrain_step";
    LinTrainArgs a = {};
    int rc = lt_net(who, n_features, B, w1, b1, heads, target_l3, workspace, &a);
    if (rc == ANTSRL_OK)
        rc = dqn_batch(who, n_features, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows,
                       idx, B, discount, grads, false, loss, workspace, &a.batch);
    if (rc == ANTSRL_OK) rc = antsrl_adam_step(who, adam_m, adam_v, step, lr, beta1, beta2, eps, &a.adam);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(antsrl_launch_lintrain(a, (hipStream_t)stream), who);
}

// ---- the steps that train layer1 (antsrl_l1train.h's frame): one body per stage over the net's descriptor, ExpNet for
// the explore agent's step (antsrl_exptrain.hip) and JointNet for the joint step (antsrl_jointtrain.hip) --------------------

template <class Net>
static int l1t_sizes(const char *who, int32_t n_features, int64_t B, size_t *trained_floats, size_t *workspace_bytes,
                     int32_t *launches)
{
    int rc = lt_features(who, n_features);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, Net::MAX_B);
    if (rc != ANTSRL_OK) return rc;
    if (trained_floats) *trained_floats = Net::floats(n_features);
    if (workspace_bytes) *workspace_bytes = l1t_workspace_bytes<Net>((int)B);
    if (launches) *launches = 2;
    return ANTSRL_OK;
}

// the nets and the workspace of the gradient stage and the fused step
template <class Net>
static int l1t_net(const char *who, int32_t n_features, int64_t B, float *model, const float *target, void *workspace,
                   L1TrainArgs *a)
{
    int rc = lt_features(who, n_features);
    if (rc == ANTSRL_OK) rc = antsrl_dqn_B(who, B, Net::MAX_B);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(model, 4);
    if ((rc = require_named(who, Net::TARGET, target, 4)) != ANTSRL_OK) return rc;
    REQUIRE(workspace, 256);
    a->model = model; a->target = target;
    a->dh = (float *)((unsigned char *)workspace + l1t_dh_offset<Net>((int)B));
    a->blocks = l1t_blocks((int)B);
    return ANTSRL_OK;
}

template <class Net>
static int l1t_grad(const char *who, int32_t n_features, const float *model, const float *target, const float *states,
                    const float *agent_states, const int64_t *actions, const float *rewards, const float *new_states,
                    const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B,
                    float discount, float *grads, float *loss, void *workspace, void *stream)
{
    L1TrainArgs a = {};
    int rc = l1t_net<Net>(who, n_features, B, const_cast<float *>(model), target, workspace, &a);
    if (rc == ANTSRL_OK)
        rc = dqn_batch(who, n_features, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows,
                       idx, B, discount, grads, true, loss, workspace, &a.batch);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(Net::launch(a, (hipStream_t)stream), who); // a.adam.on == 0: model is only read
}

template <class Net>
static int l1t_step(const char *who, int32_t n_features, float *model, const float *target, float *adam_m, float *adam_v,
                    const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                    const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                    const int64_t *idx, int64_t B, float discount, int64_t step, double lr, double beta1, double beta2,
                    double eps, float *grads, float *loss, void *workspace, void *stream)
{
    L1TrainArgs a = {};
    int rc = l1t_net<Net>(who, n_features, B, model, target, workspace, &a);
    if (rc == ANTSRL_OK)
        rc = dqn_batch(who, n_features, states, agent_states, actions, rewards, new_states, new_agent_states, dones, n_rows,
                       idx, B, discount, grads, false, loss, workspace, &a.batch);
    if (rc == ANTSRL_OK) rc = antsrl_adam_step(who, adam_m, adam_v, step, lr, beta1, beta2, eps, &a.adam);
    if (rc != ANTSRL_OK) return rc;
    return enqueued(Net::launch(a, (hipStream_t)stream), who);
}

template <class Net>
static int l1t_apply(const char *who, int32_t n_features, float *model, float *adam_m, float *adam_v, const float *grads,
                     int64_t step, double lr, double beta1, double beta2, double eps, void *stream)
{
    const int rc = lt_features(who, n_features);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(model, 4);
    return antsrl_adam_apply(who, model, adam_m, adam_v, grads, step, lr, beta1, beta2, eps, (int)Net::floats(n_features), stream);
}

extern "C" int antsrl_exptrain_sizes(int32_t n_features, int64_t B, size_t *trained_floats, size_t *workspace_bytes,
                                     int32_t *launches)
{
    return l1t_sizes<ExpNet>("exptrain_sizes", n_features, B, trained_floats, workspace_bytes, launches);
}

extern "C" int antsrl_exptrain_grad(int32_t n_features, const float *model, const float *target, const float *states,
                                    const float *agent_states, const int64_t *actions, const float *rewards,
                                    const float *new_states, const float *new_agent_states, const uint8_t *dones,
                                    int64_t n_rows, const int64_t *idx, int64_t B, float discount, float *grads, float *loss,
                                    void *workspace, void *stream)
{
    return l1t_grad<ExpNet>("exptrain_grad", n_features, model, target, states, agent_states, actions, rewards, new_states,
                            new_agent_states, dones, n_rows, idx, B, discount, grads, loss, workspace, stream);
}

extern "C" int antsrl_exptrain_apply(int32_t n_features, float *model, float *adam_m, float *adam_v, const float *grads,
                                     int64_t step, double lr, double beta1, double beta2, double eps, void *stream)
{
    return l1t_apply<ExpNet>("exptrain_apply", n_features, model, adam_m, adam_v, grads, step, lr, beta1, beta2, eps, stream);
}

extern "C" int antsrl_exptrain_step(int32_t n_features, float *model, const float *target, float *adam_m, float *adam_v,
                                    const float *states, const float *agent_states, const int64_t *actions,
                                    const float *rewards, const float *new_states, const float *new_agent_states,
                                    const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, float discount,
                                    int64_t step, double lr, double beta1, double beta2, double eps, float *grads,
                                    float *loss, void *workspace, void *stream)
{
    return l1t_step<ExpNet>("exptrain_step", n_features, model, target, adam_m, adam_v, states, agent_states, actions,
                            rewards, new_states, new_agent_states, dones, n_rows, idx, B, discount, step, lr, beta1, beta2, eps,
                            grads, loss, workspace, stream);
}

extern "C" int antsrl_jointtrain_sizes(int32_t n_features, int64_t B, size_t *trained_floats, size_t *workspace_bytes,
                                       int32_t *launches)
{
    return l1t_sizes<JointNet>("jointtrain_sizes", n_features, B, trained_floats, workspace_bytes, launches);
}

extern "C" int antsrl_jointtrain_grad(int32_t n_features, const float *model, const float *target_l3, const float *states,
                                      const float *agent_states, const int64_t *actions, const float *rewards,
                                      const float *new_states, const float *new_agent_states, const uint8_t *dones,
                                      int64_t n_rows, const int64_t *idx, int64_t B, float discount, float *grads, float *loss,
                                      void *workspace, void *stream)
{
    return l1t_grad<JointNet>("jointtrain_grad", n_features, model, target_l3, states, agent_states, actions, rewards, new_states,
                              new_agent_states, dones, n_rows, idx, B, discount, grads, loss, workspace, stream);
}

extern "C" int antsrl_jointtrain_apply(int32_t n_features, float *model, float *adam_m, float *adam_v, const float *grads,
                                       int64_t step, double lr, double beta1, double beta2, double eps, void *stream)
{
    return l1t_apply<JointNet>("jointtrain_apply", n_features, model, adam_m, adam_v, grads, step, lr, beta1, beta2, eps, stream);
}

extern "C" int antsrl_jointtrain_step(int32_t n_features, float *model, const float *target_l3, float *adam_m, float *adam_v,
                                      const float *states, const float *agent_states, const int64_t *actions,
                                      const float *rewards, const float *new_states, const float *new_agent_states,
                                      const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, float discount,
                                      int64_t step, double lr, double beta1, double beta2, double eps, float *grads,
                                      float *loss, void *workspace, void *stream)
{
    return l1t_step<JointNet>("jointtrain_step", n_features, model, target_l3, adam_m, adam_v, states, agent_states,
                              actions, rewards, new_states, new_agent_states, dones, n_rows, idx, B, discount, step, lr, beta1,
                              beta2, eps, grads, loss, workspace, stream);
}
