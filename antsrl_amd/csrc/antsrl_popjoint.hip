// antsrl_popjoint.hip — P joint agents (CollectAgent with the freeze of layer1 lifted, the curriculum's third stage) in
// lockstep on one handle: the acting net and the training step of every member in the launches of one
// (include/antsrl.h, "The population of joint agents"; antsrl_population.h holds the layout; DESIGN.md §7.28 the reasons
// and the measurements).  Select and record are the linear population's kernels (antsrl_population.hip), unchanged.
//
// As in antsrl_popexplore.hip, each kernel is the single agent's stage with the member taken from the grid: it moves the
// single agent's arguments (filled by the host for member 0) to its member and runs the single agent's own code,
//   k_pop_joint_policy<OBS16>     antsrl_policy_flat_body.inc     (k_policy_flat, both heads)     grid (blocks, P)
//   k_pop_jointtrain_fwd          antsrl_jointtrain_fwd_body.inc  (k_jointtrain_fwd)              grid (ceil(B / 128), P)
//   k_pop_jointtrain_l1           dqn_l1_stage, antsrl_dqn_dev.h  (k_jointtrain_l1)               grid (nslabs + 1, P)
// the two bodies as textual includes (antsrl_population.hip's header says why), the layer1 stage as the __device__
// function the single steps share; all three read blockIdx.x only.  So member p computes, bit for bit, what
// antsrl_policy_mlp (on JointTrainer.policy's views) and antsrl_jointtrain_step compute on its own block, rows and slab.
//
// A member's block is JointNet::floats(F) = 32 (F + 2) + 230 floats and its target layer3 99 floats, an odd
// count: blocks are 4-byte aligned and no more.  Nothing here needs more, and every read and write of a block goes float
// by float: the acting body reads w1, b1, w2, b2, w3 and b3 one float at a time (its 16-byte loads are the
// observation's); dqn_stage_w1 reads w1[row * (F + 2) + k]; the forward body's other staging loops read heads[i],
// target_l3[i], b1[hid] and the two columns behind the observation's one float each; dqn_store_adam / adam_at read and
// write params, m, v and grads at one index.  The float4 stores of dh go to the workspace, whose member stride is a
// multiple of 256 bytes (the float4 loads of the heads are LDS's).
// No atomics, no scratch; no kernel reads what another member's workgroups write; every order of sums is the single step's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_jointtrain.h"
#include "antsrl_jointtrain_dev.h"
#include "antsrl_population_dev.h"

static_assert(sizeof(PopTable) + sizeof(L1TrainArgs) + sizeof(PopRunningLoss) + 16 <= 4096, "the training kernels' arguments");

// ------------------------------------------------------------------ acting
// k_pop_policy with the joint net in its flat blocks: layer1 and layer2 are the member's LIVE model block, layer3 its
// target copy (what JointTrainer.policy views: CollectAgent.get_action acts with the target net, whose ExploreModel is
// the model's own)
template <bool OBS16>
__global__ void __launch_bounds__(POL_FLAT_THREADS)
k_pop_joint_policy(const PopJointPolicyArgs pa, const int ksteps, const int tile_elems)
{
    // the body's names, for this member
    const size_t member = blockIdx.y, rows_m = (size_t)pa.Mm, in_m = (size_t)pa.F + 2;
    const float *__restrict__ obs = reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(pa.obs) +
                                                                     member * rows_m * (size_t)pa.F * (OBS16 ? 2 : 4));
    const float *__restrict__ agent_state = pa.agent_state + member * rows_m * 2;
    const float *__restrict__ w1 = pa.model + member * JointNet::floats(pa.F), *__restrict__ b1 = w1 + JT_HIDDEN * in_m;
    const float *__restrict__ w2 = b1 + JT_HIDDEN, *__restrict__ b2 = w2 + 96;
    const float *__restrict__ w3 = pa.target_l3 + member * LT_L3, *__restrict__ b3 = w3 + 96;
    int8_t *__restrict__ rot_out = pa.rot + member * rows_m, *__restrict__ ph_out = pa.ph + member * rows_m;
    float *__restrict__ logits_out = nullptr;
    const int M = pa.Mm, F = pa.F;
#include "antsrl_policy_flat_body.inc"
}

// ------------------------------------------------------------------ training
// Grid (l1t_blocks(B) <= 4, P).  One wave per SIMD (amdgpu_waves_per_eu(1, 1)), as k_jointtrain_fwd has it
// and for the reason written above k_pop_exptrain_fwd (antsrl_popexplore.hip): a population puts up to 4 x 64 of these
// workgroups on the device, where two on one CU is no longer out of the question.  The attribute limits occupancy only:
// the arithmetic is the body's.
__global__ void __launch_bounds__(64 * JT_WAVES) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_pop_jointtrain_fwd(const L1TrainArgs a0, const PopTable tab, const unsigned ws_floats)
{
    const L1TrainArgs a = pop_l1t_member<JointNet>(a0, tab, blockIdx.y, ws_floats);
#include "antsrl_jointtrain_fwd_body.inc"
}

// Grid (nslabs + 1, P): k_jointtrain_l1 on the member's block, then the member's running loss as k_pop_exptrain_l1 keeps it
__global__ void __launch_bounds__(64 * DQN_L1_WAVES)
k_pop_jointtrain_l1(const L1TrainArgs a0, const PopTable tab, const PopRunningLoss rl, const int nslabs, const unsigned ws_floats)
{
    pop_l1t_l1_stage<JointNet>(a0, tab, rl, nslabs, ws_floats);
}

// ------------------------------------------------------------------ launchers (antsrl_population.h, antsrl_jointtrain.h)
hipError_t antsrl_launch_pop_joint_policy(const PopJointPolicyArgs &a, bool obs_bf16, hipStream_t st)
{
    return pop_policy_launch<k_pop_joint_policy<true>, k_pop_joint_policy<false>>(a, obs_bf16, st);
}

hipError_t JointNet::launch_pop(const L1TrainArgs &a, const PopTable &t, int P, size_t ws_stride, const PopRunningLoss &rl,
                                hipStream_t st)
{
    return pop_l1t_launch<JointNet, k_pop_jointtrain_fwd, k_pop_jointtrain_l1>(a, t, P, ws_stride, rl, st);
}
