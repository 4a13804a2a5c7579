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
// A member's block is ExpNet::floats(F) floats, an odd count for an even F: blocks are 4-byte aligned and no more.
// Nothing here needs more: the acting body reads w1, b1, w2 and b2 one float at a time (its 16-byte loads are the
// observation's), dqn_stage_w1 and the forward body's staging loops read the two blocks one float at a time, and
// dqn_store_adam / adam_at read and write params, m, v and grads one float at a time.  The float4 stores of dh go to the
// workspace, whose member stride is a multiple of 256 bytes.
// No atomics, no scratch; no kernel reads what another member's workgroups write; every order of sums is the single step's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_exptrain.h"
#include "antsrl_exptrain_dev.h"
#include "antsrl_population_dev.h"

static_assert(sizeof(PopTable) + sizeof(L1TrainArgs) + sizeof(PopRunningLoss) + 16 <= 4096, "the training kernels' arguments");

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
    const float *__restrict__ w1 = pa.target + member * ExpNet::floats(pa.F), *__restrict__ b1 = w1 + ET_HIDDEN * in_m;
    const float *__restrict__ w2 = b1 + ET_HIDDEN, *__restrict__ b2 = w2 + 96;
    const float *__restrict__ w3 = nullptr, *__restrict__ b3 = nullptr;
    int8_t *__restrict__ rot_out = pa.rot + member * rows_m, *__restrict__ ph_out = nullptr;
    float *__restrict__ logits_out = nullptr;
    const int M = pa.Mm, F = pa.F;
#include "antsrl_policy_flat_body.inc"
}

// ------------------------------------------------------------------ training
// Grid (l1t_blocks(B) <= 4, P).  One wave per SIMD (amdgpu_waves_per_eu(1, 1)), as k_jointtrain_fwd and
// k_lintrain: antsrl_lintrain.hip records one launch in seventeen with one workgroup's partials different when two such
// workgroups shared a CU (mechanism unknown), and none with one wave per SIMD.  k_exptrain_fwd at the agent's B = 256 is two
// workgroups on 256 CUs and has never met the condition; a population puts up to 4 x 64 of them on the device, where two
// on one CU is no longer out of the question.  The attribute limits occupancy only: the arithmetic is the body's.
__global__ void __launch_bounds__(64 * ET_WAVES) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_pop_exptrain_fwd(const L1TrainArgs a0, const PopTable tab, const unsigned ws_floats)
{
    const L1TrainArgs a = pop_l1t_member<ExpNet>(a0, tab, blockIdx.y, ws_floats);
#include "antsrl_exptrain_fwd_body.inc"
}

// Grid (nslabs + 1, P): k_exptrain_l1 on the member's block, then the member's running loss as k_pop_lintrain keeps it
__global__ void __launch_bounds__(64 * DQN_L1_WAVES)
k_pop_exptrain_l1(const L1TrainArgs a0, const PopTable tab, const PopRunningLoss rl, const int nslabs, const unsigned ws_floats)
{
    pop_l1t_l1_stage<ExpNet>(a0, tab, rl, nslabs, ws_floats);
}

// ------------------------------------------------------------------ launchers (antsrl_population.h, antsrl_exptrain.h)
hipError_t antsrl_launch_pop_explore_policy(const PopExplorePolicyArgs &a, bool obs_bf16, hipStream_t st)
{
    return pop_policy_launch<k_pop_explore_policy<true>, k_pop_explore_policy<false>>(a, obs_bf16, st);
}

hipError_t ExpNet::launch_pop(const L1TrainArgs &a, const PopTable &t, int P, size_t ws_stride, const PopRunningLoss &rl,
                              hipStream_t st)
{
    return pop_l1t_launch<ExpNet, k_pop_exptrain_fwd, k_pop_exptrain_l1>(a, t, P, ws_stride, rl, st);
}
