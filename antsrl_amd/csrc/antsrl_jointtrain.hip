// antsrl_jointtrain.hip — the DQN training step of CollectModel with layer1 trained under the collect heads (the
// reference's CollectAgent.train with the freeze of layer1 lifted: layer1 and layer2 live in model and target net, layer3
// with a target copy) as TWO launches.  include/antsrl.h ("The joint training step") holds the contract,
// antsrl_jointtrain.h the layout of the net's block, DESIGN.md §7.21 the reasons.
//
// Stage 1 (k_jointtrain_fwd), one wave per 32 minibatch rows, four waves per workgroup, one tile per wave:
// k_exptrain_fwd's shape (antsrl_exptrain.hip) with ONE bf16 image of the live W1 in LDS for both h and h', and
// k_lintrain's four head evaluations (antsrl_lintrain.hip) behind it in fp32 on the fp32 masters: the model's layer2 on h,
// the same live layer2 on h', the model's layer3 on h, the target's layer3 on h'.  Then the two TD targets,
// d = q[a] - y and dq = d * 2 / (3 B) per head, and
//     dh[b][j] = dq_rot[b] * w2[a_rot][j] + dq_ph[b] * w3[a_ph][j]     two fp32 products and one add, each rounded on its
// own, in that order, stored to the workspace.  The wave leaves h (with a column of ones for the biases) and dq (with the
// row's loss term) in its LDS tile, and lane l sums outputs l, l + 64, l + 128, l + 192 of the 199 (the 198 head gradients
// in the flat block's order, the loss) over the tile's 32 rows in row order from zero; the workgroup adds its four waves'
// sums in wave order and writes them to its row of the partials.
// Stage 2 (k_jointtrain_l1): dqn_l1_stage (antsrl_dqn_dev.h), the body k_exptrain_l1 runs, on this net's block: the
// [32][F + 3] product dh^T xe in column slabs with Adam in place, and one more workgroup that adds stage 1's partials in
// workgroup order, writes the 198 head gradients and the loss and runs Adam on the heads.
// No atomics anywhere and every order above is fixed: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_dqn_dev.h"
#include "antsrl_jointtrain.h"
#include "antsrl_jointtrain_dev.h"
#include "antsrl_lds_optin.h"

// One wave per SIMD, as k_lintrain (antsrl_lintrain.hip): this is that kernel's forward at up to 512
// workgroups, and the condition under which it once returned a differing row of partials is a second wave on the SIMD.
// The body is one text (antsrl_jointtrain_fwd_body.inc), run for every member of a population by k_pop_jointtrain_fwd
// (antsrl_popjoint.hip) too.
__global__ void __launch_bounds__(64 * JT_WAVES) __attribute__((amdgpu_waves_per_eu(1, 1))) k_jointtrain_fwd(const JointTrainArgs a)
{
#include "antsrl_jointtrain_fwd_body.inc"
}

// the layer1 stage: dqn_l1_stage (antsrl_dqn_dev.h) on CollectModel's block, b1 behind w1 and the 198 heads behind b1
__global__ void __launch_bounds__(64 * DQN_L1_WAVES) k_jointtrain_l1(const JointTrainArgs a, const int nslabs)
{
    __shared__ float red[DQN_L1_WAVES * JT_HIDDEN * DQN_L1_SLAB];
    const size_t ob1 = (size_t)JT_HIDDEN * (a.batch.F + 2);
    dqn_l1_stage(a.batch, a.model, a.adam, a.dh, a.blocks, nslabs, DqnL1Layout{ob1, ob1 + JT_HIDDEN, JT_OUT, JT_PART}, red);
}

hipError_t antsrl_launch_jointtrain(const JointTrainArgs &a, hipStream_t st)
{
    const size_t lds = jt_lds(a.batch.ksteps); // 45 760 bytes at F = 294, 91 840 at the widest rows: above 64 KiB it is an opt-in per device
    hipError_t e = antsrl_lds_optin<k_jointtrain_fwd>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_jointtrain_fwd, dim3(a.blocks), dim3(64 * JT_WAVES), lds, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int nslabs = (a.batch.F + 3 + DQN_L1_SLAB - 1) / DQN_L1_SLAB;
    hipLaunchKernelGGL(k_jointtrain_l1, dim3(nslabs + 1), dim3(64 * DQN_L1_WAVES), 0, st, a, nslabs);
    return hipGetLastError();
}
