// antsrl_popexplore.hip — P explore agents in lockstep on one handle: the acting net and the training step of every
// member in the launches of one (include/antsrl.h, "The population of explore agents"; antsrl_population.h holds the
// layout; DESIGN.md §7.25 the reasons and the measurements).  Select and record are the linear population's kernels
// (antsrl_population.hip): the record body writes (rotation + 1, 1) for a NULL pheromone.
//
// As there, each kernel is the single agent's stage with the member taken from the grid: it moves the single agent's
// arguments (filled by the host for member 0) to its member and runs the single agent's own code,
//   k_pop_explore_policy<OBS16>   antsrl_policy_flat_body.inc    (k_policy_flat, w3 = NULL)   grid (blocks, P)
//   k_pop_exptrain_fwd            antsrl_exptrain_fwd_body.inc   (k_exptrain_fwd)             grid (ceil(B / 128), P)
//   k_pop_exptrain_l1             dqn_l1_stage, antsrl_dqn_dev.h (k_exptrain_l1)              grid (nslabs + 1, P)
// the two bodies as textual includes (antsrl_population.hip's header says why), the layer1 stage as the __device__
// function it has been since the joint step shares it; both read blockIdx.x only.  So member p computes, bit for bit,
// what antsrl_policy_mlp (without a pheromone head) and antsrl_exptrain_step compute on its own block, rows and slab.
//
// A member's block is antsrl_exptrain_floats(F) floats, an odd count for an even F: blocks are 4-byte aligned and no more.
// Nothing here needs more: the acting body reads w1, b1, w2 and b2 one float at a time (its 16-byte loads are the
// observation's), dqn_stage_w1 and the forward body's staging loops read the two blocks one float at a time, and
// dqn_store_adam / adam_at read and write params, m, v and grads one float at a time.  The float4 stores of dh go to the
// workspace, whose member stride is a multiple of 256 bytes.
// No atomics, no scratch; no kernel reads what another member's workgroups write; every order of sums is the single step's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_dqn_dev.h"
#include "antsrl_exptrain.h"
#include "antsrl_exptrain_dev.h"
#include "antsrl_lds_optin.h"
#include "antsrl_policy_flat.h"
#include "antsrl_population.h"

static_assert(sizeof(PopTable) + sizeof(ExpTrainArgs) + sizeof(PopRunningLoss) + 16 <= 4096, "the training kernels' arguments");

// ------------------------------------------------------------------ acting
// k_pop_policy with the explore net: the four tensors are the member's TARGET block (ExploreTrainer's acting net is the
// target net), there is no pheromone head and nothing writes a pheromone.
template <bool OBS16>
__global__ void __launch_bounds__(POL_FLAT_THREADS)
k_pop_explore_policy(const PopExplorePolicyArgs pa, const int ksteps, const int tile_elems)
{
    // the body's names, for this member
    const size_t member = blockIdx.y, rows_m = (size_t)pa.Mm, in_m = (size_t)pa.F + 2;
    const float *__restrict__ obs = reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(pa.obs) +
                                                                     member * rows_m * (size_t)pa.F * (OBS16 ? 2 : 4));
    const float *__restrict__ agent_state = pa.agent_state + member * rows_m * 2;
    const float *__restrict__ w1 = pa.target + member * antsrl_exptrain_floats(pa.F), *__restrict__ b1 = w1 + ET_HIDDEN * in_m;
    const float *__restrict__ w2 = b1 + ET_HIDDEN, *__restrict__ b2 = w2 + 96;
    const float *__restrict__ w3 = nullptr, *__restrict__ b3 = nullptr;
    int8_t *__restrict__ rot_out = pa.rot + member * rows_m, *__restrict__ ph_out = nullptr;
    float *__restrict__ logits_out = nullptr;
    const int M = pa.Mm, F = pa.F;
#include "antsrl_policy_flat_body.inc"
}

// ------------------------------------------------------------------ training
// ws_floats: floats between two members' parts of the workspace (antsrl_pop_exptrain_stride / 4)
__device__ __forceinline__ ExpTrainArgs pop_exptrain_member(const ExpTrainArgs &a0, const PopTable &tab, const size_t member,
                                                            const size_t ws_floats)
{
    const size_t L = (size_t)a0.batch.n_rows, F = (size_t)a0.batch.F, NF = antsrl_exptrain_floats(a0.batch.F);
    ExpTrainArgs a = a0;
    a.model = a0.model + member * NF;
    a.target = a0.target + member * NF;
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

// Grid (antsrl_exptrain_blocks(B) <= 4, P).  One wave per SIMD (amdgpu_waves_per_eu(1, 1)), as k_jointtrain_fwd and
// k_lintrain: antsrl_lintrain.hip records one launch in seventeen with one workgroup's partials different when two such
// workgroups shared a CU (mechanism unknown), and none with one wave per SIMD.  k_exptrain_fwd at the agent's B = 256 is two
// workgroups on 256 CUs and has never met the condition; a population puts up to 4 x 64 of them on the device, where two
// on one CU is no longer out of the question.  The attribute limits occupancy only: the arithmetic is the body's.
__global__ void __launch_bounds__(64 * ET_WAVES) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_pop_exptrain_fwd(const ExpTrainArgs a0, const PopTable tab, const unsigned ws_floats)
{
    const ExpTrainArgs a = pop_exptrain_member(a0, tab, blockIdx.y, ws_floats);
#include "antsrl_exptrain_fwd_body.inc"
}

// Grid (nslabs + 1, P): k_exptrain_l1 on the member's block, then the member's running loss as k_pop_lintrain keeps it
__global__ void __launch_bounds__(64 * ET_L1_WAVES)
k_pop_exptrain_l1(const ExpTrainArgs a0, const PopTable tab, const PopRunningLoss rl, const int nslabs, const unsigned ws_floats)
{
    __shared__ float red[ET_L1_WAVES * ET_HIDDEN * ET_SLAB];
    const ExpTrainArgs a = pop_exptrain_member(a0, tab, blockIdx.y, ws_floats);
    const size_t ob1 = (size_t)ET_HIDDEN * (a.batch.F + 2);
    dqn_l1_stage(a.batch, a.model, a.adam, a.dh, a.blocks, nslabs, DqnL1Layout{ob1, ob1 + ET_HIDDEN, ET_OUT, ET_PART}, red);
    // main.py:106-109 in float64, antsrl_monitor.hip's arithmetic (each product rounded before the add: the build's
    // -ffp-contract=off), by the thread that has just written the member's loss (dqn_l1_stage: thread nout - 1 of
    // workgroup nslabs)
    if (rl.running_loss && (int)blockIdx.x == nslabs && threadIdx.x == ET_OUT - 1) {
        const double l = (double)*a.batch.loss;
        rl.running_loss[blockIdx.y] = rl.first ? l : 0.99 * rl.running_loss[blockIdx.y] + 0.01 * l;
    }
}

// ------------------------------------------------------------------ launchers (antsrl_population.h)
hipError_t antsrl_launch_pop_explore_policy(const PopExplorePolicyArgs &a, bool obs_bf16, hipStream_t st)
{
    if (a.Mm < 1 || a.P < 1 || !pol_flat_fits(a.F)) return hipErrorInvalidValue;
    const int ks = (a.F + 15) / 16, tile_elems = pol_flat_tile_elems(a.F);
    size_t lds = 0;
    const int blocks = pop_policy_blocks(a.Mm, a.F, a.P, &lds); // k_pop_policy's launch rule
    const hipError_t e = obs_bf16 ? antsrl_lds_optin<k_pop_explore_policy<true>>(lds)
                                  : antsrl_lds_optin<k_pop_explore_policy<false>>(lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)blocks, (unsigned)a.P);
    if (obs_bf16)
        hipLaunchKernelGGL(k_pop_explore_policy<true>, grid, dim3(POL_FLAT_THREADS), lds, st, a, ks, tile_elems);
    else
        hipLaunchKernelGGL(k_pop_explore_policy<false>, grid, dim3(POL_FLAT_THREADS), lds, st, a, ks, tile_elems);
    return hipGetLastError();
}

hipError_t antsrl_launch_pop_exptrain(const ExpTrainArgs &a, const PopTable &t, int P, size_t ws_stride,
                                      const PopRunningLoss &rl, hipStream_t st)
{
    // (the entry refuses B > 512 in words.)  The stride holds a member's partials and dh and keeps them 256-byte aligned
    if (P < 1 || P > ANTSRL_POP_MAX || a.blocks < 1 || a.blocks > 4 || a.blocks != antsrl_exptrain_blocks(a.batch.B) ||
        ws_stride % 256 || ws_stride < antsrl_pop_exptrain_stride(a.batch.B))
        return hipErrorInvalidValue;
    const size_t lds = et_lds(a.batch.ksteps);
    hipError_t e = antsrl_lds_optin<k_pop_exptrain_fwd>(lds);
    if (e != hipSuccess) return e;
    const unsigned ws_floats = (unsigned)(ws_stride / sizeof(float));
    hipLaunchKernelGGL(k_pop_exptrain_fwd, dim3((unsigned)a.blocks, (unsigned)P), dim3(64 * ET_WAVES), lds, st, a, t, ws_floats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int nslabs = (a.batch.F + 3 + ET_SLAB - 1) / ET_SLAB;
    hipLaunchKernelGGL(k_pop_exptrain_l1, dim3((unsigned)(nslabs + 1), (unsigned)P), dim3(64 * ET_L1_WAVES), 0, st, a, t, rl,
                       nslabs, ws_floats);
    return hipGetLastError();
}
