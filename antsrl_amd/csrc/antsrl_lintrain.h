// antsrl_lintrain.h — the on-device DQN training step of the linear agent's net (antsrl_lintrain.hip), shared with its
// C-ABI entries (antsrl_linapi.hip).  The net is CollectModel over ExploreModel (agents/collect_agent.py:24-51): layer1
// [32][F + 2] frozen, layer2 [3][32] (rotation) and layer3 [3][32] (pheromone) trained.
//
// HEADS is the flat fp32 block of the 198 trained floats, in the state_dict's order:
//   w2 [3][32] at 0, b2 [3] at 96, w3 [3][32] at 99, b3 [3] at 195
// and the target net's layer3 is the 99 floats  w3 [3][32] at 0, b3 [3] at 96.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_fail.h"

#define LT_HIDDEN 32
#define LT_HEADS 198       // trained floats
#define LT_L3 99           // floats of one layer3
#define LT_OUT 199         // the 198 gradients and the loss
#define LT_PART 200        // floats per workgroup in the partials (LT_OUT rounded up)
#define LT_FUSED_TILES 16  // up to this many 32-row tiles, one workgroup (4 waves, up to 4 tiles each) does the whole step
#define LT_MAX_BLOCKS 1024 // workgroups of 4 waves otherwise (tiles are looped)

struct LinTrainArgs {
    const float *states, *agent_states, *rewards, *new_states, *new_agent_states;
    const int64_t *actions, *idx; // actions [N][2]; idx [B] or NULL (rows 0 .. B - 1)
    const uint8_t *dones;
    const float *w1, *b1;     // the frozen layer1
    float *heads;             // LT_HEADS floats: read by the forward, written by Adam
    const float *target_l3;   // LT_L3 floats
    float *m, *v;             // Adam's moments, LT_HEADS floats each (adam only)
    float *grads;             // LT_HEADS floats, or NULL
    float *loss;              // one float
    float *partials;          // [workgroups][LT_PART] (more than one workgroup only)
    long long n_rows;         // rows of the replay arrays: idx is clamped to [0, n_rows)
    int B, F, ksteps, ntiles;
    float discount, dq_scale /* 2 / (3 B) */, loss_scale /* 1 / (3 B) */;
    int adam;                 // 0: gradients and loss only
    float step_size, bc2_sqrt, w1m, beta2, w2m, eps;
};

// workgroups of the gradient stage for B rows (1: the step is one launch)
ANTSRL_INTERNAL int antsrl_lintrain_blocks(int B, int F);
// the gradient stage, and behind it (more than one workgroup) the finish: at most two launches
ANTSRL_INTERNAL hipError_t antsrl_launch_lintrain(const LinTrainArgs &a, hipStream_t st);
// Adam alone from a.grads (a.heads, a.m, a.v and the Adam scalars are read)
ANTSRL_INTERNAL hipError_t antsrl_launch_lintrain_apply(const LinTrainArgs &a, hipStream_t st);
