// antsrl_l1train.h — the frame of a DQN training step that trains layer1, stated once for the nets that run on it: the
// explore step (antsrl_exptrain.h) and the joint step (antsrl_jointtrain.h).  Two launches.  A forward stage (the net's
// own: its body is a textual include) takes 32 minibatch rows per wave, L1T_WAVES waves per workgroup, and writes one row
// of partial sums per workgroup and dh [B][32] into one workspace; dqn_l1_stage (antsrl_dqn_dev.h) then takes layer1's
// gradient in column slabs with Adam in place and adds the partials.  The workspace is
//   partials [blocks(B)][Net::PART] floats at 0, dh [B][32] floats at dh_offset(B) (256-byte aligned)
// and a population's is that per member, a member's part rounded up to 256 bytes.
//
// What differs between two nets is the forward body and a descriptor `Net`, a struct of
//   OUT, PART           outputs of the forward stage (the head gradients and the loss), floats per row of the partials
//   MAX_B, POP_MAX_B    the largest minibatch of a single step and of a population's member
//   TARGET              the ABI's name of the target pointer, for messages
//   floats(F)           floats of a net's flat block [w1 [32][F + 2] | b1 [32] | the heads]
//   target_floats(F)    floats of what the target owns (per member of a population)
//   lds(ksteps)         the forward stage's dynamic LDS (defined beside the body's LDS layout, antsrl_*train_dev.h)
//   launch, launch_pop  the step's two launches for one net and for a population (defined beside the kernels)
// Everything below, antsrl_l1train_dev.h, the entries' bodies in antsrl_linapi.hip and antsrl_popapi.hip take it as a
// template parameter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_adam.h"
#include "antsrl_dqn.h"
#include "antsrl_fail.h"

#define L1T_WAVES 4 // waves per workgroup of a forward stage: it takes 4 tiles of 32 rows

struct PopTable;       // antsrl_population.h
struct PopRunningLoss;

struct L1TrainArgs {
    DqnBatch batch;      // grads: floats(F) floats; partials: [workgroups of the forward stage][PART]
    float *model;        // floats(F) floats: read by the forward, written by Adam
    const float *target; // target_floats(F) floats, only read
    float *dh;           // workspace: [B][32]
    int blocks;          // workgroups of the forward stage
    AdamArgs adam;       // m, v: floats(F) floats each
};

// floats of a flat block whose layer1 is [32][F + 2] with `behind` floats of heads behind b1
__host__ __device__ static inline size_t l1t_floats(int F, int behind) { return (size_t)DQN_HIDDEN * (F + 2) + DQN_HIDDEN + behind; }

static inline int l1t_blocks(int B) { return ((B + 31) / 32 + L1T_WAVES - 1) / L1T_WAVES; }
static inline int l1t_nslabs(int F) { return (F + 3 + DQN_L1_SLAB - 1) / DQN_L1_SLAB; }
// bytes of the partials in front of dh in the workspace (256-byte aligned)
template <class Net>
static inline size_t l1t_dh_offset(int B) { return ((size_t)l1t_blocks(B) * Net::PART * 4 + 255) / 256 * 256; }
template <class Net>
static inline size_t l1t_workspace_bytes(int B) { return l1t_dh_offset<Net>(B) + (size_t)B * DQN_HIDDEN * sizeof(float); }
// bytes of a member's part of a population's workspace: the single step's rounded up to 256, so that every member's
// partials and dh start as aligned as the single step's (B * 128 is no multiple of 256 for odd B)
template <class Net>
static inline size_t l1t_pop_stride(int B) { return (l1t_workspace_bytes<Net>(B) + 255) / 256 * 256; }
