// antsrl_rework.h — the rework agent's net on the device (antsrl_rework.hip), shared with its C-ABI entries
// (antsrl_reworkapi.hip).  The net is CollectModelRework (agents/collect_agent_rework.py:24-63): ten nn.Linear layers and
// no activation, so both heads are one affine map of x = cat[obs.view(F), agent_state(2)], D = F + 2:
//     q = Wc x + bc,   Wc [NQ][D], bc [NQ],   NQ = n_rot + n_ph, the rotation rows first.
//
// COLLAPSED is the flat fp32 buffer  Wc [NQ][D] at 0,  bc [NQ] at NQ * D  (floats): what k_rework_collapse writes and
// k_rework_act reads (with or without the epsilon-greedy select inside: ReworkSelect).
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

struct __attribute__((packed, aligned(4))) RwF4 { float v[4]; }; // 4-byte aligned 16-byte load

// what the kernels' bodies (antsrl_rework_collapse_body.inc, antsrl_rework_act_body.inc) share with whoever includes them
#define RW_TPB 256
#define RW_U 2              // sets of four rows a wave has in flight
#define RW_G 4              // chunks of a row whose loads are issued together
#define RW_MAX_BLOCKS 1024  // 4 workgroups per CU, what 120 VGPRs admit; rows beyond are looped

typedef float rw_f32x2 __attribute__((ext_vector_type(2)));

// inputs of layer l in the state_dict's order (its outputs are the inputs of the layer above it)
__device__ __forceinline__ int rw_in(const ReworkDims &d, int l)
{
    switch (l) {
    case 0: return d.D;
    case 1: return d.g1;
    case 2: return d.g2;
    case 3: return d.g3;
    case 4: return d.D;
    case 5: return d.r1;
    case 6: return d.r2;
    case 7: return d.r3;
    case 8: return d.D;
    default: return d.p1;
    }
}

// a + (a of the lane that CTRL names), by a DPP move inside the row of 16 lanes
template <int CTRL>
__device__ __forceinline__ float rw_add_dpp(float a)
{
    const int other = __builtin_amdgcn_update_dpp(0, __float_as_int(a), CTRL, 0xf, 0xf, false);
    return a + __int_as_float(other);
}

// the sum over a group of 16 lanes, in every lane of it: l ^ 1, l ^ 2, 7 - l within eight, 15 - l
__device__ __forceinline__ float rw_group_sum(float a)
{
    a = rw_add_dpp<0xB1>(a);  // quad_perm [1, 0, 3, 2]
    a = rw_add_dpp<0x4E>(a);  // quad_perm [2, 3, 0, 1]
    a = rw_add_dpp<0x141>(a); // row_half_mirror
    a = rw_add_dpp<0x140>(a); // row_mirror
    return a;
}

// epsilon-greedy behind the forward pass (antsrl_policy_rework_select): antsrl_agent_select_actions' arguments
struct ReworkSelect {
    uint64_t seed, step;
    double epsilon;
    uint8_t *explored; // [n_envs] or NULL
    uint32_t env_base, n_ants;
};

// one launch each
ANTSRL_INTERNAL hipError_t antsrl_launch_rework_collapse(const ReworkParams &P, const ReworkDims &d, float *collapsed,
                                                         hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_rework_act(const float *collapsed, const ReworkDims &d, const void *obs,
                                                    bool obs_bf16, const float *agent_state, int M, int8_t *rot, int8_t *ph,
                                                    float *q_out, hipStream_t st);
// M = n_envs * sel.n_ants rows
ANTSRL_INTERNAL hipError_t antsrl_launch_rework_act_select(const float *collapsed, const ReworkDims &d, const void *obs,
                                                           bool obs_bf16, const float *agent_state, int M,
                                                           const ReworkSelect &sel, int8_t *rot, int8_t *ph, float *q_out,
                                                           hipStream_t st);
