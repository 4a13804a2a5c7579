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
#include "antsrl_l1train.h"

#define ET_HIDDEN DQN_HIDDEN
#define ET_L2 99            // floats of layer2: w2 [3][32], b2 [3]
#define ET_OUT 100          // what the forward stage sums over rows: layer2's 99 gradients and the loss
#define ET_PART 104         // floats per workgroup in the partials (ET_OUT rounded up to 16 bytes)
#define ET_WAVES L1T_WAVES  // waves per workgroup of the forward stage

// the step on antsrl_l1train.h's frame: L1TrainArgs with a target of floats(F) floats, the full copy
struct ANTSRL_INTERNAL ExpNet {
    static constexpr int OUT = ET_OUT, PART = ET_PART;
    static constexpr int MAX_B = 65536, POP_MAX_B = 32 * ET_WAVES * 4; // a member's: four forward workgroups, the linear members' 512 rows
    static constexpr const char *TARGET = "target";
    __host__ __device__ static size_t floats(int F) { return l1t_floats(F, ET_L2); }
    __host__ __device__ static size_t target_floats(int F) { return floats(F); }
    static size_t lds(int ksteps);
    static hipError_t launch(const L1TrainArgs &a, hipStream_t st);
    // a: member 0's (B <= POP_MAX_B; idx [P][B]; partials and dh inside member 0's part of the workspace); the table
    // gives discount and step size
    static hipError_t launch_pop(const L1TrainArgs &a, const PopTable &t, int P, size_t ws_stride, const PopRunningLoss &rl,
                                 hipStream_t st);
};
