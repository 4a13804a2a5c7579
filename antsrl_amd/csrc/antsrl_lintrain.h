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
#include "antsrl_adam.h"
#include "antsrl_dqn.h"
#include "antsrl_fail.h"

#define LT_HIDDEN DQN_HIDDEN
#define LT_HEADS 198       // trained floats
#define LT_L3 99           // floats of one layer3
#define LT_OUT 199         // the 198 gradients and the loss
#define LT_PART 200        // floats per workgroup in the partials (LT_OUT rounded up)
#define LT_FUSED_TILES 16  // up to this many 32-row tiles, one workgroup (4 waves, up to 4 tiles each) does the whole step
#define LT_MAX_BLOCKS 1024 // workgroups of 4 waves otherwise (tiles are looped)

struct LinTrainArgs {
    DqnBatch batch;           // grads: LT_HEADS floats; partials: [workgroups][LT_PART] (more than one workgroup only)
    const float *w1, *b1;     // the frozen layer1
    float *heads;             // LT_HEADS floats: read by the forward, written by Adam
    const float *target_l3;   // LT_L3 floats
    AdamArgs adam;            // m, v: LT_HEADS floats each
};

// workgroups of the gradient stage for B rows (1: the step is one launch)
ANTSRL_INTERNAL int antsrl_lintrain_blocks(int B, int F);
// the gradient stage, and behind it (more than one workgroup) the finish: at most two launches
ANTSRL_INTERNAL hipError_t antsrl_launch_lintrain(const LinTrainArgs &a, hipStream_t st);
