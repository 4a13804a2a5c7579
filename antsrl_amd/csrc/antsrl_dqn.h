// antsrl_dqn.h — what every on-device DQN training step over a 32-wide layer1 takes from the replay arrays, whichever
// net it trains: the minibatch (DqnBatch, checked and filled by antsrl_linapi.hip's dqn_batch) in front of the net's own
// pointers in LinTrainArgs (antsrl_lintrain.h) and ExpTrainArgs (antsrl_exptrain.h), with Adam's part (AdamArgs,
// antsrl_adam.h) behind it.  antsrl_dqn_dev.h holds the device code the two steps share.
#pragma once
#include <stdint.h>

#define DQN_HIDDEN 32 // layer1's outputs

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
