// antsrl_l1train_dev.h — the device and launch side of antsrl_l1train.h's frame, for the translation units that hold a
// net's kernels (antsrl_exptrain.hip, antsrl_jointtrain.hip; the populations' add antsrl_population_dev.h): the body of
// a layer1 stage's kernel and the step's two launches, over the net's descriptor.  The kernels themselves stay
// __global__ functions of their own in their files, a forward body included inside each.
#pragma once
#include <hip/hip_runtime.h>
#include "antsrl_dqn_dev.h"
#include "antsrl_l1train.h"
#include "antsrl_lds_optin.h"

// the body of a layer1 stage's kernel (64 * DQN_L1_WAVES threads, nslabs + 1 workgroups): dqn_l1_stage on Net's flat
// block, b1 behind w1 and the heads behind b1
template <class Net>
__device__ __forceinline__ void l1t_l1_stage(const L1TrainArgs &a, const int nslabs)
{
    __shared__ float red[DQN_L1_WAVES * DQN_HIDDEN * DQN_L1_SLAB];
    const size_t ob1 = (size_t)DQN_HIDDEN * (a.batch.F + 2);
    dqn_l1_stage(a.batch, a.model, a.adam, a.dh, a.blocks, nslabs, DqnL1Layout{ob1, ob1 + DQN_HIDDEN, Net::OUT, Net::PART}, red);
}

// the forward stage and the layer1 stage: two launches.  Fwd's dynamic LDS is above 64 KiB at wide rows: an opt-in per device
template <class Net, auto Fwd, auto L1>
static inline hipError_t l1t_launch(const L1TrainArgs &a, hipStream_t st)
{
    const size_t lds = Net::lds(a.batch.ksteps);
    hipError_t e = antsrl_lds_optin<Fwd>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Fwd, dim3(a.blocks), dim3(64 * L1T_WAVES), lds, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int nslabs = l1t_nslabs(a.batch.F);
    hipLaunchKernelGGL(L1, dim3(nslabs + 1), dim3(64 * DQN_L1_WAVES), 0, st, a, nslabs);
    return hipGetLastError();
}
