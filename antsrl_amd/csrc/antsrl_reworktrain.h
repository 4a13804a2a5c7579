// antsrl_reworktrain.h — the on-device DQN training step of the rework agent's net (antsrl_reworktrain.hip), shared with
// its C-ABI entries (antsrl_reworkapi.hip).  The net is CollectModelRework (antsrl_rework.h): ten nn.Linear layers and no
// activation, so the loss's gradient has rank NQ = n_rot + n_ph in every weight (include/antsrl.h, "The rework agent's
// training step").  A net is ONE flat fp32 block: the 20 tensors of the state_dict in its order, dense.
//
// The minibatch's fields lie in ReworkTrainArgs under DqnBatch's names (antsrl_dqn.h), so antsrl_dqn_minibatch checks
// and fills them and dqn_row clamps idx for this step as for the 32-wide nets'; that struct's ksteps, ntiles and the fixed
// 3 in dq_scale are theirs alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_adam.h"
#include "antsrl_dqn.h"
#include "antsrl_fail.h"
#include "antsrl_rework.h"

#define RT_ROWS 16        // minibatch rows a workgroup of the batch pass takes at a time: four per wave
#define RT_MAX_PARTS 256  // workgroups of the batch pass, one partial each (rows beyond are looped)
#define RT_MAX_B 65536
#define RT_TPB 256        // threads of every workgroup of the step
#define RT_INFO 8 // floats of a row's hand-over in LDS: g_rot, g_ph, d_rot^2, d_ph^2, a_rot, n_rot + a_ph (int), the replay row (int64)

// where everything lies: floats into a parameter block, bytes into the workspace (every part 256-byte aligned)
struct ReworkTrainLayout {
    int out[RW_LAYERS], in[RW_LAYERS];  // of layer l
    int src[RW_LAYERS];                 // the layer that feeds l (-1: x)
    int k0[RW_LAYERS], k1[RW_LAYERS];   // the pseudo-rows [k0, k1) that reach l: its head's
    size_t off[2 * RW_LAYERS + 1];      // tensor t of the block (weight 2 l, bias 2 l + 1); off[20] = P
    size_t collapsed;                   // float [NQ][D], [NQ]: the MODEL's collapsed buffer
    size_t M[RW_LAYERS];                // double [NQ][out_l]
    size_t partials;                    // float [parts][part_stride]
    size_t G;                           // float [NQ][D], then s float [NQ]
    size_t A[RW_LAYERS];                // double [NQ][out_l] (none for a head's last layer: A[l] = 0 there)
    size_t bytes;
    int parts, part_stride;             // part_stride = NQ D + NQ + 2 rounded up to 64 floats
};

struct ReworkTrainArgs {
    ReworkDims d;
    ReworkTrainLayout L;
    const float *states, *agent_states, *rewards, *new_states, *new_agent_states;
    const int64_t *actions, *idx; // actions [N][2]; idx [B] or NULL (rows 0 .. B - 1)
    const uint8_t *dones;
    float *grads;                 // P floats, or NULL
    float *loss;                  // one float
    unsigned char *work;          // the workspace
    long long n_rows;             // rows of the replay arrays: idx is clamped to [0, n_rows)
    int B;
    float discount, dq_rot /* 2 / (n_rot B) */, dq_ph, loss_rot /* 1 / (n_rot B) */, loss_ph;
    float *model;                 // P floats: read by the down chain, written by Adam
    const float *target;          // the target net's collapsed buffer (the acting policy's)
    AdamArgs adam;                // m, v: P floats each
};

// host arithmetic only
ANTSRL_INTERNAL void antsrl_reworktrain_layout(const ReworkDims &d, int B, ReworkTrainLayout *L);
// the four launches: down chain, batch pass, up chain, gradient (and Adam where a.adam.on)
ANTSRL_INTERNAL hipError_t antsrl_launch_reworktrain(const ReworkTrainArgs &a, hipStream_t st);
