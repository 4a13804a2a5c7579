// antsrl_rework.h — the rework agent's net on the device (antsrl_rework.hip), shared with its C-ABI entries
// (antsrl_reworkapi.hip).  The net is CollectModelRework (agents/collect_agent_rework.py:24-63): ten nn.Linear layers and
// no activation, so both heads are one affine map of x = cat[obs.view(F), agent_state(2)], D = F + 2:
//     q = Wc x + bc,   Wc [NQ][D], bc [NQ],   NQ = n_rot + n_ph, the rotation rows first.
//
// COLLAPSED is the flat fp32 buffer  Wc [NQ][D] at 0,  bc [NQ] at NQ * D  (floats): what k_rework_collapse writes and
// k_rework_act reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_fail.h"

#define RW_LAYERS 10    // layer1..4, rotation_layer1..4, pheromone_layer1..2: the state_dict's order
#define RW_MAX_D 1024   // inputs of the net
#define RW_MAX_H 256    // width of a hidden layer
#define RW_MAX_HEAD 8   // outputs of one head

struct ReworkDims {
    int F, D, g1, g2, g3, r1, r2, r3, p1, n_rot, n_ph;
};

struct ReworkParams {
    const float *p[2 * RW_LAYERS]; // the 20 tensors of CollectModelRework.state_dict(), in its order (weight, bias per layer)
};

// one launch each
ANTSRL_INTERNAL hipError_t antsrl_launch_rework_collapse(const ReworkParams &P, const ReworkDims &d, float *collapsed,
                                                         hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_rework_act(const float *collapsed, const ReworkDims &d, const void *obs,
                                                    bool obs_bf16, const float *agent_state, int M, int8_t *rot, int8_t *ph,
                                                    float *q_out, hipStream_t st);
