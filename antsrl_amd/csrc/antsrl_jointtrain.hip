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
#include "antsrl_jointtrain.h"
#include "antsrl_jointtrain_dev.h"
#include "antsrl_l1train_dev.h"

// One wave per SIMD, as k_lintrain (antsrl_lintrain.hip): this is that kernel's forward at up to 512
// workgroups, and the condition under which it once returned a differing row of partials is a second wave on the SIMD.
// The body is one text (antsrl_jointtrain_fwd_body.inc), run for every member of a population by k_pop_jointtrain_fwd
// (antsrl_popjoint.hip) too.
__global__ void __launch_bounds__(64 * JT_WAVES) __attribute__((amdgpu_waves_per_eu(1, 1))) k_jointtrain_fwd(const L1TrainArgs a)
{
#include "antsrl_jointtrain_fwd_body.inc"
}

// the layer1 stage: dqn_l1_stage (antsrl_dqn_dev.h) on CollectModel's block, b1 behind w1 and the 198 heads behind b1
__global__ void __launch_bounds__(64 * DQN_L1_WAVES) k_jointtrain_l1(const L1TrainArgs a, const int nslabs)
{
    l1t_l1_stage<JointNet>(a, nslabs);
}

// (the forward stage's LDS: 45 760 bytes at F = 294, 91 840 at the widest rows)
hipError_t JointNet::launch(const L1TrainArgs &a, hipStream_t st) { return l1t_launch<JointNet, k_jointtrain_fwd, k_jointtrain_l1>(a, st); }
