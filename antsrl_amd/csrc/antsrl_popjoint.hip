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
// A member's block is antsrl_jointtrain_floats(F) = 32 (F + 2) + 230 floats and its target layer3 99 floats, an odd
// count: blocks are 4-byte aligned and no more.  Nothing here needs more, and every read and write of a block goes float
// by float: the acting body reads w1, b1, w2, b2, w3 and b3 one float at a time (its 16-byte loads are the
// observation's); dqn_stage_w1 reads w1[row * (F + 2) + k]; the forward body's other staging loops read heads[i],
// target_l3[i], b1[hid] and the two columns behind the observation's one float each; dqn_store_adam / adam_at read and
// write params, m, v and grads at one index.  The float4 stores of dh go to the workspace, whose member stride is a
// multiple of 256 bytes (the float4 loads of the heads are LDS's).
// No atomics, no scratch; no kernel reads what another member's workgroups write; every order of sums is the single step's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_dqn_dev.h"
#include "antsrl_jointtrain.h"
#include "antsrl_jointtrain_dev.h"
#include "antsrl_lds_optin.h"
#include "antsrl_policy_flat.h"
#include "antsrl_population.h"

static_assert(sizeof(PopTable) + sizeof(JointTrainArgs) + sizeof(PopRunningLoss) + 16 <= 4096, "the training kernels' arguments");

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
    const float *__restrict__ w1 = pa.model + member * antsrl_jointtrain_floats(pa.F), *__restrict__ b1 = w1 + JT_HIDDEN * in_m;
    const float *__restrict__ w2 = b1 + JT_HIDDEN, *__restrict__ b2 = w2 + 96;
    const float *__restrict__ w3 = pa.target_l3 + member * LT_L3, *__restrict__ b3 = w3 + 96;
    int8_t *__restrict__ rot_out = pa.rot + member * rows_m, *__restrict__ ph_out = pa.ph + member * rows_m;
    float *__restrict__ logits_out = nullptr;
    const int M = pa.Mm, F = pa.F;
#include "antsrl_policy_flat_body.inc"
}

// ------------------------------------------------------------------ training
// ws_floats: floats between two members' parts of the workspace (antsrl_pop_jointtrain_stride / 4)
__device__ __forceinline__ JointTrainArgs pop_jointtrain_member(const JointTrainArgs &a0, const PopTable &tab, const size_t member,
                                                                const size_t ws_floats)
{
    const size_t L = (size_t)a0.batch.n_rows, F = (size_t)a0.batch.F, NF = antsrl_jointtrain_floats(a0.batch.F);
    JointTrainArgs a = a0;
    a.model = a0.model + member * NF;
    a.target_l3 = a0.target_l3 + member * LT_L3;
    a.adam.m = a0.adam.m + member * NF;
    a.adam.v = a0.adam.v + member * NF;
    a.adam.step_size = tab.m[member].step_size;
    a.dh = a0.dh + member * ws_floats;
    DqnBatch &mb = a.batch;
    mb.states = a0.batch.states + member * L * F;
    mb.new_states = a0.batch.new_states + member * L * F;
    mb.agent_states = a0.batch.agent_states + member * L * 2;
    mb.new_agent_states = a0.batch.new_agent_states + member * L * 2;
    mb.actions = a0.batch.actions + member * L * 2;
    mb.rewards = a0.batch.rewards + member * L;
    mb.dones = a0.batch.dones + member * L;
    mb.idx = a0.batch.idx + member * (size_t)a0.batch.B;
    mb.grads = a0.batch.grads ? a0.batch.grads + member * NF : nullptr;
    mb.loss = a0.batch.loss + member;
    mb.partials = a0.batch.partials + member * ws_floats;
    mb.discount = tab.m[member].discount;
    return a;
}

// Grid (antsrl_jointtrain_blocks(B) <= 4, P).  One wave per SIMD (amdgpu_waves_per_eu(1, 1)), as k_jointtrain_fwd has it
// and for the reason written above k_pop_exptrain_fwd (antsrl_popexplore.hip): a population puts up to 4 x 64 of these
// workgroups on the device, where two on one CU is no longer out of the question.  The attribute limits occupancy only:
// the arithmetic is the body's.
__global__ void __launch_bounds__(64 * JT_WAVES) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_pop_jointtrain_fwd(const JointTrainArgs a0, const PopTable tab, const unsigned ws_floats)
{
    const JointTrainArgs a = pop_jointtrain_member(a0, tab, blockIdx.y, ws_floats);
#include "antsrl_jointtrain_fwd_body.inc"
}

// Grid (nslabs + 1, P): k_jointtrain_l1 on the member's block, then the member's running loss as k_pop_exptrain_l1 keeps it
__global__ void __launch_bounds__(64 * DQN_L1_WAVES)
k_pop_jointtrain_l1(const JointTrainArgs a0, const PopTable tab, const PopRunningLoss rl, const int nslabs, const unsigned ws_floats)
{
    __shared__ float red[DQN_L1_WAVES * JT_HIDDEN * DQN_L1_SLAB];
    const JointTrainArgs a = pop_jointtrain_member(a0, tab, blockIdx.y, ws_floats);
    const size_t ob1 = (size_t)JT_HIDDEN * (a.batch.F + 2);
    dqn_l1_stage(a.batch, a.model, a.adam, a.dh, a.blocks, nslabs, DqnL1Layout{ob1, ob1 + JT_HIDDEN, JT_OUT, JT_PART}, red);
    // main.py:106-109 in float64, antsrl_monitor.hip's arithmetic (each product rounded before the add: the build's
    // -ffp-contract=off), by the thread that has just written the member's loss (dqn_l1_stage: thread nout - 1 of
    // workgroup nslabs)
    if (rl.running_loss && (int)blockIdx.x == nslabs && threadIdx.x == JT_OUT - 1) {
        const double l = (double)*a.batch.loss;
        rl.running_loss[blockIdx.y] = rl.first ? l : 0.99 * rl.running_loss[blockIdx.y] + 0.01 * l;
    }
}

// ------------------------------------------------------------------ launchers (antsrl_population.h)
hipError_t antsrl_launch_pop_joint_policy(const PopJointPolicyArgs &a, bool obs_bf16, hipStream_t st)
{
    if (a.Mm < 1 || a.P < 1 || !pol_flat_fits(a.F)) return hipErrorInvalidValue;
    const int ks = (a.F + 15) / 16, tile_elems = pol_flat_tile_elems(a.F);
    size_t lds = 0;
    const int blocks = pop_policy_blocks(a.Mm, a.F, a.P, &lds); // k_pop_policy's launch rule
    const hipError_t e = obs_bf16 ? antsrl_lds_optin<k_pop_joint_policy<true>>(lds)
                                  : antsrl_lds_optin<k_pop_joint_policy<false>>(lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)blocks, (unsigned)a.P);
    if (obs_bf16)
        hipLaunchKernelGGL(k_pop_joint_policy<true>, grid, dim3(POL_FLAT_THREADS), lds, st, a, ks, tile_elems);
    else
        hipLaunchKernelGGL(k_pop_joint_policy<false>, grid, dim3(POL_FLAT_THREADS), lds, st, a, ks, tile_elems);
    return hipGetLastError();
}

hipError_t antsrl_launch_pop_jointtrain(const JointTrainArgs &a, const PopTable &t, int P, size_t ws_stride,
                                        const PopRunningLoss &rl, hipStream_t st)
{
    // (the entry refuses B > 512 in words.)  The stride holds a member's partials and dh and keeps them 256-byte aligned
    if (P < 1 || P > ANTSRL_POP_MAX || a.blocks < 1 || a.blocks > 4 || a.blocks != antsrl_jointtrain_blocks(a.batch.B) ||
        ws_stride % 256 || ws_stride < antsrl_pop_jointtrain_stride(a.batch.B))
        return hipErrorInvalidValue;
    const size_t lds = jt_lds(a.batch.ksteps);
    hipError_t e = antsrl_lds_optin<k_pop_jointtrain_fwd>(lds);
    if (e != hipSuccess) return e;
    const unsigned ws_floats = (unsigned)(ws_stride / sizeof(float));
    hipLaunchKernelGGL(k_pop_jointtrain_fwd, dim3((unsigned)a.blocks, (unsigned)P), dim3(64 * JT_WAVES), lds, st, a, t, ws_floats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int nslabs = (a.batch.F + 3 + DQN_L1_SLAB - 1) / DQN_L1_SLAB;
    hipLaunchKernelGGL(k_pop_jointtrain_l1, dim3((unsigned)(nslabs + 1), (unsigned)P), dim3(64 * DQN_L1_WAVES), 0, st, a, t, rl,
                       nslabs, ws_floats);
    return hipGetLastError();
}
