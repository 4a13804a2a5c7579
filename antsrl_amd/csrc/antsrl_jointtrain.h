// antsrl_jointtrain.h — the on-device DQN training step of CollectModel with layer1 trained under the collect heads
// (antsrl_jointtrain.hip), shared with its C-ABI entries (antsrl_linapi.hip).  The net is CollectModel over ExploreModel
// (agents/collect_agent.py:24-51) with the freeze of layer1 lifted and nothing else changed: model and target net share
// one ExploreModel, so layer1 and layer2 are live in both and only layer3 has a target copy.
//
// A net is ONE flat fp32 block of P = 32 (F + 2) + 32 + 198 floats in CollectModel.state_dict()'s order:
//   w1 [32][F + 2] at 0, b1 [32] at 32 (F + 2), then the linear step's 198-float heads block (antsrl_lintrain.h):
//   w2 [3][32] at 32 (F + 2) + 32, b2 [3] at + 128, w3 [3][32] at + 131, b3 [3] at + 227
// and Adam's m and v and the gradient are laid out the same way.  The target net's layer3 is 99 floats of its own.
//
// Precision: antsrl_exptrain.h's.  Both layer1 passes (h and h', through the ONE bf16 image of the live w1) round x and w1
// to bfloat16; the gradient of layer1 is the straight-through one, bf16 x against the fp32 master.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_adam.h"
#include "antsrl_dqn.h"
#include "antsrl_fail.h"
#include "antsrl_lintrain.h"

#define JT_HIDDEN DQN_HIDDEN
#define JT_HEADS LT_HEADS   // floats behind layer1: w2, b2, w3, b3
#define JT_OUT LT_OUT       // what the forward stage sums over rows: the 198 head gradients and the loss
#define JT_PART LT_PART     // floats per workgroup in the partials: k_lintrain's [200] row
#define JT_WAVES 4          // waves per workgroup of the forward stage: it takes 4 tiles of 32 rows
#define JT_MAX_B 65536      // rows of a minibatch

struct JointTrainArgs {
    DqnBatch batch;           // grads: P floats; partials: [workgroups of the forward stage][JT_PART]
    float *model;             // P floats: read by the forward, written by Adam
    const float *target_l3;   // LT_L3 floats, only read
    float *dh;                // workspace: [B][32]
    int blocks;               // workgroups of the forward stage
    AdamArgs adam;            // m, v: P floats each
};

__host__ __device__ static inline size_t antsrl_jointtrain_floats(int F) { return (size_t)JT_HIDDEN * (F + 2) + JT_HIDDEN + JT_HEADS; }
static inline int antsrl_jointtrain_blocks(int B) { return ((B + 31) / 32 + JT_WAVES - 1) / JT_WAVES; }
// bytes of the partials in front of dh in the workspace (256-byte aligned)
static inline size_t antsrl_jointtrain_dh_offset(int B) { return ((size_t)antsrl_jointtrain_blocks(B) * JT_PART * 4 + 255) / 256 * 256; }

// the forward stage and the layer1 stage: two launches
ANTSRL_INTERNAL hipError_t antsrl_launch_jointtrain(const JointTrainArgs &a, hipStream_t st);
