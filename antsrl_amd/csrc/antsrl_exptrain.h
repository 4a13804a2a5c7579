// antsrl_exptrain.h — the on-device DQN training step of ExploreModel (antsrl_exptrain.hip), shared with its C-ABI
// entries (antsrl_linapi.hip).  The net is agents/explore_agent_pytorch.py:24-45 with the concat of
// agents/collect_agent.py:47-49: layer1 [32][F + 2] and layer2 [3][32], BOTH trained; the target net is a full copy.
//
// A net is ONE flat fp32 block of P = 32 (F + 2) + 32 + 96 + 3 floats in the state_dict's order:
//   w1 [32][F + 2] at 0, b1 [32] at 32 (F + 2), w2 [3][32] at 32 (F + 2) + 32, b2 [3] at 32 (F + 2) + 128
// and Adam's m and v and the gradient are laid out the same way.
//
// Precision.  Both layer1 passes round x and w1 to bfloat16, as the acting kernel does; the gradient of layer1 is taken
// with that bfloat16-rounded x against the fp32 master w1 (a straight-through gradient: the rounding of w1 is treated as
// the identity).  An Adam step at lr 1e-4 is about one bfloat16 ulp of a weight of size 0.05, so most single steps do not
// change the rounded weight: they accumulate in the fp32 master and reach the forward pass when the master crosses a
// rounding boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_adam.h"
#include "antsrl_dqn.h"
#include "antsrl_fail.h"

#define ET_HIDDEN DQN_HIDDEN
#define ET_L2 99            // floats of layer2: w2 [3][32], b2 [3]
#define ET_OUT 100          // what the forward stage sums over rows: layer2's 99 gradients and the loss
#define ET_PART 104         // floats per workgroup in the partials (ET_OUT rounded up to 16 bytes)
#define ET_WAVES 4          // waves per workgroup of the forward stage: it takes 4 tiles of 32 rows
#define ET_L1_WAVES DQN_L1_WAVES // waves per workgroup of the layer1 stage: wave w walks rows w, w + 16, ...
#define ET_MAX_B 65536      // rows of a minibatch
#define ET_SLAB DQN_L1_SLAB // columns of layer1 one workgroup of the layer1 stage owns

struct ExpTrainArgs {
    DqnBatch batch;           // grads: P floats; partials: [workgroups of the forward stage][ET_PART]
    float *model;             // P floats: read by the forward, written by Adam
    const float *target;      // P floats, only read
    float *dh;                // workspace: [B][32]
    int blocks;               // workgroups of the forward stage
    AdamArgs adam;            // m, v: P floats each
};

__host__ __device__ static inline size_t antsrl_exptrain_floats(int F) { return (size_t)ET_HIDDEN * (F + 2) + ET_HIDDEN + ET_L2; }
static inline int antsrl_exptrain_blocks(int B) { return ((B + 31) / 32 + ET_WAVES - 1) / ET_WAVES; }
// bytes of the partials in front of dh in the workspace (256-byte aligned)
static inline size_t antsrl_exptrain_dh_offset(int B) { return ((size_t)antsrl_exptrain_blocks(B) * ET_PART * 4 + 255) / 256 * 256; }

// the forward stage and the layer1 stage: two launches
ANTSRL_INTERNAL hipError_t antsrl_launch_exptrain(const ExpTrainArgs &a, hipStream_t st);
