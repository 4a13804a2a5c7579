// antsrl_dqn.h — what every on-device DQN training step takes from the replay arrays, whichever net it trains.  The
// minibatch's fields carry one set of names in DqnBatch (below: the 32-wide nets', in front of the net's own pointers in
// LinTrainArgs, antsrl_lintrain.h, and L1TrainArgs, antsrl_l1train.h) and in ReworkTrainArgs (antsrl_reworktrain.h),
// so one host function checks and fills them for every entry (antsrl_dqn_minibatch) and one device function clamps idx
// into the ring (dqn_row).  Adam's part is AdamArgs (antsrl_adam.h); antsrl_dqn_dev.h holds the device code the two
// 32-wide steps share.
#pragma once
#include <stdint.h>
#include "antsrl_fail.h"

#define DQN_HIDDEN 32 // layer1's outputs
// the layer1 stage the steps that train layer1 share (dqn_l1_stage, antsrl_dqn_dev.h)
#define DQN_L1_WAVES 16 // waves per workgroup: wave w walks rows w, w + 16, ...
#define DQN_L1_SLAB 8   // columns of the [32][F + 3] product one workgroup owns

struct DqnBatch {
    const float *states, *agent_states, *rewards, *new_states, *new_agent_states;
    const int64_t *actions, *idx; // actions [N][2]; idx [B] or NULL (rows 0 .. B - 1)
    const uint8_t *dones;
    float *grads;             // the trained floats' gradients, or NULL
    float *loss;              // one float
    float *partials;          // workspace: [workgroups][floats per workgroup]
    long long n_rows;         // rows of the replay arrays: idx is clamped to [0, n_rows)
    int B, F, ksteps, ntiles;
    float discount, dq_scale /* 2 / (3 B) */, loss_scale /* 1 / (3 B) */;
};

// a minibatch's rows against its entry's limit, for the explore, the joint and the rework step and the population's
// members (the linear step's limit is an INVALID one with its own words, lt_B): 1 <= B <= max_B; `limit`, where the
// entry gives one, says behind the second refusal what of a member's step max_B rows are
static inline int antsrl_dqn_B(const char *who, int64_t B, int max_B, const char *limit = nullptr)
{
    if (B < 1) return fail(ANTSRL_E_INVALID, "%s: B must be >= 1 (%lld)", who, (long long)B);
    if (B > max_B)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: B = %lld > %d rows%s%s", who, (long long)B, max_B,
                    limit ? ": a member's step is " : "", limit ? limit : "");
    return ANTSRL_OK;
}

// the minibatch of a gradient stage or a fused step, for a B its entry has checked: the replay arrays, idx, grads, loss
// and the discount into the fields of *q that carry their names (Q: DqnBatch or ReworkTrainArgs), or the refusal.  The
// net, the workspace and the scales stay with the entry.
template <class Q>
static inline int antsrl_dqn_minibatch(const char *who, const float *states, const float *agent_states,
                                       const int64_t *actions, const float *rewards, const float *new_states,
                                       const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                                       const int64_t *idx, int64_t B, float discount, float *grads, bool grads_required,
                                       float *loss, Q *q)
{
    if (n_rows < 1 || n_rows > (1LL << 40)) return fail(ANTSRL_E_INVALID, "%s: n_rows must be in [1, 2^40] (%lld)", who, (long long)n_rows);
    if (!idx && B > n_rows) return fail(ANTSRL_E_INVALID, "%s: without idx, B = %lld rows need n_rows >= B (%lld)", who, (long long)B, (long long)n_rows);
    REQUIRE(states, 4);
    REQUIRE(agent_states, 4);
    REQUIRE(actions, 8);
    REQUIRE(rewards, 4);
    REQUIRE(new_states, 4);
    REQUIRE(new_agent_states, 4);
    REQUIRE(dones, 1);
    if ((uintptr_t)idx & 7) return fail(ANTSRL_E_INVALID, "%s: idx must be 8-byte aligned", who);
    if (grads_required && !grads) return fail(ANTSRL_E_INVALID, "%s: grads is required", who);
    if ((uintptr_t)grads & 3) return fail(ANTSRL_E_INVALID, "%s: grads must be 4-byte aligned", who);
    REQUIRE(loss, 4);
    if (!(discount == discount)) return fail(ANTSRL_E_INVALID, "%s: discount is NaN", who);
    q->states = states; q->agent_states = agent_states; q->rewards = rewards; q->new_states = new_states;
    q->new_agent_states = new_agent_states; q->actions = actions; q->idx = idx; q->dones = dones;
    q->grads = grads; q->loss = loss;
    q->n_rows = n_rows;
    q->B = (int)B;
    q->discount = discount;
    return ANTSRL_OK;
}

// The 32-wide nets' rules, for the single agents' entries and the population's (antsrl_linapi.hip): 1 <= n_features,
// n_features + 2 <= 1024; and antsrl_dqn_minibatch's part of *q followed by F, ksteps, ntiles, the two scales and the
// partials (= workspace, NULL where a step is one workgroup per net), for n_features and B the entry has checked
ANTSRL_INTERNAL int lt_features(const char *who, int32_t n_features);
ANTSRL_INTERNAL int dqn_batch(const char *who, int32_t n_features, const float *states, const float *agent_states,
                              const int64_t *actions, const float *rewards, const float *new_states,
                              const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx,
                              int64_t B, float discount, float *grads, bool grads_required, float *loss, void *workspace,
                              DqnBatch *q);

// the replay row of minibatch row b (b < B), never outside the replay arrays
template <class Q>
__device__ __forceinline__ long long dqn_row(const Q &q, const int b)
{
    const long long ri = q.idx ? q.idx[b] : (long long)b;
    return ri < 0 ? 0 : (ri >= q.n_rows ? q.n_rows - 1 : ri);
}
