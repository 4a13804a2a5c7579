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
#include "antsrl_l1train.h"
#include "antsrl_lintrain.h"

#define JT_HIDDEN DQN_HIDDEN
#define JT_HEADS LT_HEADS   // floats behind layer1: w2, b2, w3, b3
#define JT_OUT LT_OUT       // what the forward stage sums over rows: the 198 head gradients and the loss
#define JT_PART LT_PART     // floats per workgroup in the partials: k_lintrain's [200] row
#define JT_WAVES L1T_WAVES  // waves per workgroup of the forward stage

// the step on antsrl_l1train.h's frame: L1TrainArgs whose target is the target net's layer3, LT_L3 floats
struct ANTSRL_INTERNAL JointNet {
    static constexpr int OUT = JT_OUT, PART = JT_PART;
    static constexpr int MAX_B = 65536, POP_MAX_B = 32 * JT_WAVES * 4; // a member's: the explore member's four forward workgroups
    static constexpr const char *TARGET = "target_l3";
    __host__ __device__ static size_t floats(int F) { return l1t_floats(F, JT_HEADS); }
    __host__ __device__ static size_t target_floats(int) { return LT_L3; }
    static size_t lds(int ksteps);
    static hipError_t launch(const L1TrainArgs &a, hipStream_t st);
    // a: member 0's, as ExpNet::launch_pop's (antsrl_exptrain.h)
    static hipError_t launch_pop(const L1TrainArgs &a, const PopTable &t, int P, size_t ws_stride, const PopRunningLoss &rl,
                                 hipStream_t st);
};
