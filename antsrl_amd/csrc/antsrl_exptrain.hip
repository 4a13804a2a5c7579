// antsrl_exptrain.hip — the DQN training step of ExploreModel (layer1 [32][F + 2] and layer2 [3][32], both trained; the
// target net a full copy) as TWO launches.  include/antsrl.h ("The explore agent's training step") holds the contract,
// antsrl_exptrain.h the layout of a net's block, DESIGN.md §7.12 the reasons.
//
// Stage 1 (k_exptrain_fwd), one wave per 32 minibatch rows, four waves per workgroup.  It is k_lintrain's forward
// (antsrl_lintrain.hip) with two bf16 images of W1 in LDS, the model's for h and the target's for h' (both fit at every
// supported width: 129 KB of the 160 at F = 1022, so there is no second code path for wide rows): lane (r, h) gathers row
// idx[r] of states / new_states, rounds it to bf16 and multiplies it with the image by v_mfma_f32_32x32x16_bf16 over the
// 16-input steps in ascending order from a zero accumulator, then  acc + (as0 * w1[.][F] + as1 * w1[.][F + 1]) + b1  in
// fp32 on bf16-rounded operands: the acting kernel's sequence.  Behind that everything is fp32 on the fp32 masters: q and
// q', the TD target, d = q[a] - y, dq = d * 2 / (3 B), and
//     dh[b][j] = dq[b] * w2[a_b][j]             one fp32 product, stored to the workspace as it is.
// The wave leaves h (with a column of ones for b2) and dq (with the row's loss term) in its LDS tile, and lane l sums
// outputs l and l + 64 of the 100 (layer2's 99 gradients, the loss) over the tile's 32 rows in row order from zero; the
// workgroup adds its four waves' sums in wave order and writes them to its row of the partials.
// Stage 2 (k_exptrain_l1: dqn_l1_stage, antsrl_dqn_dev.h, shared with the joint step).  Workgroup s < S = ceil((F + 3) / 8) owns columns 8 s .. 8 s + 7 of the [32][F + 3] product
//     g[j][k] = sum_b dh[b][j] * xe[b][k],      xe[b] = bf16(states[i_b]) ++ bf16(agent_states[i_b]) ++ 1
// (columns 0 .. F + 1 are g_w1, column F + 2 is g_b1).  Lane (j, c) = (lane & 31, lane >> 5) of wave w keeps the four
// columns 8 s + 4 c .. + 3 of hidden unit j and walks rows w, w + 16, w + 32, ... (16 waves) in ascending order, one fmaf per
// row and column from zero, eight rows' loads in flight: the stage is bound by the latency of its dependent loads (idx[b],
// then the row), so it wants rows in flight, not arithmetic.  The 16 waves' sums are then added in wave order from wave
// 0's, (((w0 + w1) + w2) + ...) + w15.  The same workgroup
// writes the gradient and runs Adam on its own columns, so nothing crosses workgroups.  Workgroup S adds stage 1's
// partials in workgroup order, writes layer2's gradient and the loss and runs Adam on layer2.
// No atomics anywhere and every order above is fixed: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_exptrain.h"
#include "antsrl_exptrain_dev.h"
#include "antsrl_l1train_dev.h"

// the forward stage: its body is one text (antsrl_exptrain_fwd_body.inc), run for every member of a population by
// k_pop_exptrain_fwd (antsrl_popexplore.hip) too
__global__ void __launch_bounds__(64 * ET_WAVES) k_exptrain_fwd(const L1TrainArgs a)
{
#include "antsrl_exptrain_fwd_body.inc"
}

// the layer1 stage: dqn_l1_stage (antsrl_dqn_dev.h) on ExploreModel's block, b1 behind w1 and layer2 behind b1
__global__ void __launch_bounds__(64 * DQN_L1_WAVES) k_exptrain_l1(const L1TrainArgs a, const int nslabs)
{
    l1t_l1_stage<ExpNet>(a, nslabs);
}

// (the forward stage's LDS: 61 KB at F = 294, 151 KB at the widest rows)
hipError_t ExpNet::launch(const L1TrainArgs &a, hipStream_t st) { return l1t_launch<ExpNet, k_exptrain_fwd, k_exptrain_l1>(a, st); }
