// antsrl_population_dev.h — what the populations' training and acting kernels share on the device and at their launch
// (antsrl_population.hip, antsrl_popexplore.hip, antsrl_popjoint.hip): the move of a minibatch's ring arrays and of a
// layer1-trained step's arguments from member 0 to a member, the body of a population's layer1 stage with the running
// loss behind it, the two launches of a population's layer1-trained step (antsrl_l1train.h's frame on a grid (x, P))
// and the launch of a flat acting kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "antsrl_l1train_dev.h"
#include "antsrl_policy_flat.h"
#include "antsrl_population.h"

// Member 0's minibatch b0 moved to `member` in mb (a copy of b0), as far as every step moves it alike: the ring's seven
// arrays by the member's L rows of F features, idx by B.  grads, loss, partials and discount stay with the caller, behind
// this in the order the kernels have always had them (k_pop_lintrain compiles to other code when a statement moves).
// Q, Q0: DqnBatch, or the rework step's arguments, which carry the minibatch under the same names (antsrl_dqn.h).
template <class Q, class Q0>
__device__ __forceinline__ void pop_ring_member(Q &mb, const Q0 &b0, const size_t member, const size_t L, const size_t F)
{
    mb.states = b0.states + member * L * F;
    mb.new_states = b0.new_states + member * L * F;
    mb.agent_states = b0.agent_states + member * L * 2;
    mb.new_agent_states = b0.new_agent_states + member * L * 2;
    mb.actions = b0.actions + member * L * 2;
    mb.rewards = b0.rewards + member * L;
    mb.dones = b0.dones + member * L;
    mb.idx = b0.idx + member * (size_t)b0.B;
}

// The arguments of a layer1-trained step for `member`, from member 0's.  ws_floats: floats between two members' parts of
// the workspace (l1t_pop_stride / 4)
template <class Net>
__device__ __forceinline__ L1TrainArgs pop_l1t_member(const L1TrainArgs &a0, const PopTable &tab, const size_t member,
                                                      const size_t ws_floats)
{
    const size_t L = (size_t)a0.batch.n_rows, F = (size_t)a0.batch.F, NF = Net::floats(a0.batch.F);
    L1TrainArgs a = a0;
    a.model = a0.model + member * NF;
    a.target = a0.target + member * Net::target_floats(a0.batch.F);
    a.adam.m = a0.adam.m + member * NF;
    a.adam.v = a0.adam.v + member * NF;
    a.adam.step_size = tab.m[member].step_size;
    a.dh = a0.dh + member * ws_floats;
    pop_ring_member(a.batch, a0.batch, member, L, F);
    a.batch.grads = a0.batch.grads ? a0.batch.grads + member * NF : nullptr;
    a.batch.loss = a0.batch.loss + member;
    a.batch.partials = a0.batch.partials + member * ws_floats;
    a.batch.discount = tab.m[member].discount;
    return a;
}

// The arguments of the rework net's step (antsrl_reworktrain.h) for `member`, from member 0's: the model block, Adam's
// moments and the gradients by the block's floats, the target (the member's collapsed buffer) by a buffer's floats, the
// ring and idx as every step moves them, loss by one float, the workspace by ws_stride bytes (a multiple of 256, at
// least a0.L.bytes); discount and Adam's step size from the table.  The layout a.L is every member's: it is the single
// step's for the same B.
//
// What comes back is PopReworkTrainArgs: ReworkTrainArgs under the names the bodies read, with `d` and `L` REFERENCES to
// member 0's, where the kernel's arguments hold them.  The bodies index L's arrays by a layer they compute; a moved copy
// of the whole struct is then an array in scratch (808 bytes a thread in the down, up and gradient kernels), a reference
// leaves the tables in the argument segment as the single kernels have them.
struct PopReworkTrainArgs {
    const ReworkDims &d;
    const ReworkTrainLayout &L;
    const float *states, *agent_states, *rewards, *new_states, *new_agent_states;
    const int64_t *actions, *idx;
    const uint8_t *dones;
    float *grads, *loss;
    unsigned char *work;
    long long n_rows;
    int B;
    float discount, dq_rot, dq_ph, loss_rot, loss_ph;
    float *model;
    const float *target;
    AdamArgs adam;
};

__device__ __forceinline__ PopReworkTrainArgs pop_rt_member(const ReworkTrainArgs &a0, const PopTable &tab, const size_t member,
                                                            const size_t ws_stride)
{
    const size_t L = (size_t)a0.n_rows, F = (size_t)a0.d.F, NF = a0.L.off[2 * RW_LAYERS];
    const size_t CF = (size_t)(a0.d.n_rot + a0.d.n_ph) * (size_t)(a0.d.D + 1);
    PopReworkTrainArgs a = {a0.d, a0.L, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, a0.n_rows, a0.B, 0.0f, a0.dq_rot, a0.dq_ph, a0.loss_rot, a0.loss_ph, nullptr, nullptr, a0.adam};
    a.model = a0.model + member * NF;
    a.target = a0.target + member * CF;
    a.adam.m = a0.adam.m + member * NF;
    a.adam.v = a0.adam.v + member * NF;
    a.adam.step_size = tab.m[member].step_size;
    pop_ring_member(a, a0, member, L, F);
    a.grads = a0.grads ? a0.grads + member * NF : nullptr;
    a.loss = a0.loss + member;
    a.work = a0.work + member * ws_stride;
    a.discount = tab.m[member].discount;
    return a;
}

// The body of a population's layer1 stage (grid (nslabs + 1, P)): the single step's on the member's block, then the
// member's running loss as k_pop_lintrain keeps it: main.py:106-109 in float64, antsrl_monitor.hip's arithmetic (each
// product rounded before the add: the build's -ffp-contract=off), by the thread that has just written the member's loss
// (dqn_l1_stage: thread OUT - 1 of workgroup nslabs)
template <class Net>
__device__ __forceinline__ void pop_l1t_l1_stage(const L1TrainArgs &a0, const PopTable &tab, const PopRunningLoss &rl,
                                                 const int nslabs, const unsigned ws_floats)
{
    const L1TrainArgs a = pop_l1t_member<Net>(a0, tab, blockIdx.y, ws_floats);
    l1t_l1_stage<Net>(a, nslabs);
    if (rl.running_loss && (int)blockIdx.x == nslabs && threadIdx.x == Net::OUT - 1) {
        const double l = (double)*a.batch.loss;
        rl.running_loss[blockIdx.y] = rl.first ? l : 0.99 * rl.running_loss[blockIdx.y] + 0.01 * l;
    }
}

// l1t_launch for a population: Fwd on a grid (blocks <= 4, P), L1 on (nslabs + 1, P)
template <class Net, auto Fwd, auto L1>
static inline hipError_t pop_l1t_launch(const L1TrainArgs &a, const PopTable &t, int P, size_t ws_stride, const PopRunningLoss &rl,
                                        hipStream_t st)
{
    // (the entry refuses B > 512 in words.)  The stride holds a member's partials and dh and keeps them 256-byte aligned
    if (P < 1 || P > ANTSRL_POP_MAX || a.blocks < 1 || a.blocks > 4 || a.blocks != l1t_blocks(a.batch.B) || ws_stride % 256 ||
        ws_stride < l1t_pop_stride<Net>(a.batch.B))
        return hipErrorInvalidValue;
    const size_t lds = Net::lds(a.batch.ksteps);
    hipError_t e = antsrl_lds_optin<Fwd>(lds);
    if (e != hipSuccess) return e;
    const unsigned ws_floats = (unsigned)(ws_stride / sizeof(float));
    hipLaunchKernelGGL(Fwd, dim3((unsigned)a.blocks, (unsigned)P), dim3(64 * L1T_WAVES), lds, st, a, t, ws_floats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int nslabs = l1t_nslabs(a.batch.F);
    hipLaunchKernelGGL(L1, dim3((unsigned)(nslabs + 1), (unsigned)P), dim3(64 * DQN_L1_WAVES), 0, st, a, t, rl, nslabs, ws_floats);
    return hipGetLastError();
}

// The launch of a flat acting kernel (Bf16, F32: its two instantiations by the observation's format) on Args' Mm rows
// per member: the LDS opt-in, the grid from pop_policy_blocks (antsrl_population.h)
template <auto Bf16, auto F32, class Args>
static inline hipError_t pop_policy_launch(const Args &a, bool obs_bf16, hipStream_t st)
{
    if (a.Mm < 1 || a.P < 1 || !pol_flat_fits(a.F)) return hipErrorInvalidValue;
    const int ks = (a.F + 15) / 16, tile_elems = pol_flat_tile_elems(a.F);
    size_t lds = 0;
    const int blocks = pop_policy_blocks(a.Mm, a.F, a.P, &lds);
    const hipError_t e = obs_bf16 ? antsrl_lds_optin<Bf16>(lds) : antsrl_lds_optin<F32>(lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)blocks, (unsigned)a.P);
    if (obs_bf16)
        hipLaunchKernelGGL(Bf16, grid, dim3(POL_FLAT_THREADS), lds, st, a, ks, tile_elems);
    else
        hipLaunchKernelGGL(F32, grid, dim3(POL_FLAT_THREADS), lds, st, a, ks, tile_elems);
    return hipGetLastError();
}
