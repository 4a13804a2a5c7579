// antsrl_population.h — a population of P linear agents trained in lockstep on one handle (include/antsrl.h, "The
// population of linear agents"): what antsrl_population.hip's kernels take and their launchers, shared with the C-ABI
// entries (antsrl_popapi.hip).
//
// Member p owns environments [p Em, (p + 1) Em) of the handle's n_envs = P Em, i.e. ants [p Mm, (p + 1) Mm), Mm = Em n_ants.
// Every per-member device tensor is member-major, a member's block laid out as the single agent's: w1 [P][32][F + 2],
// b1 [P][32], heads [P][198], target_l3 [P][99], adam [P][2][198], grads [P][198], loss [P], and the ring's seven arrays
// with a leading [P].  A kernel takes the single agent's argument struct filled for MEMBER 0 and moves it to its own
// member (from the grid) before it runs the single agent's body: the pointers by the member's stride, the seed, epsilon,
// discount and Adam step size from the table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_adam.h"
#include "antsrl_exptrain.h"
#include "antsrl_fail.h"
#include "antsrl_jointtrain.h"
#include "antsrl_lintrain.h"
#include "antsrl_memagent.h"
#include "antsrl_memtrain.h"
#include "antsrl_policy_flat.h"
#include "antsrl_reworktrain.h"

// The members' hyper-parameters: host values that travel BY VALUE in the kernel arguments (as EnvCopyTable does,
// antsrl_checkpoint.h), so a changed epsilon costs no device allocation and no copy.  24 bytes x 64 = 1.5 KB.
struct PopMember {
    uint64_t seed;
    double epsilon;
    float discount;
    float step_size; // Adam's lr / (1 - beta1^step), from the member's learning rate (antsrl_adam_args)
};
struct PopTable {
    PopMember m[ANTSRL_POP_MAX];
};

// the acting net of every member on its Mm rows: grid (blocks, P)
struct PopPolicyArgs {
    const void *obs;          // [P][Mm][F], float32 or bfloat16, dense
    const float *agent_state; // [P][Mm][2]
    const float *w1, *b1, *heads, *target_l3;
    int8_t *rot, *ph;         // [P][Mm]
    int Mm, F, P;
};

// the running loss behind the step (main.py:106-109 per member), or running_loss == NULL
struct PopRunningLoss {
    double *running_loss; // [P]
    int first;            // this is the first training step: running_loss[p] = loss[p]
};

// ---- the population of explore agents (antsrl_popexplore.hip; include/antsrl.h, "The population of explore agents") ----
// A member's net is ExploreTrainer's flat block of ExpNet::floats(F) floats (antsrl_exptrain.h): model, target,
// Adam's m and v and grads are [P][floats].  The count is odd for an even F (9603 at F = 294), so a member's block starts
// 4-byte aligned and no more: every kernel reads and writes the blocks float by float.

// the acting net of every member, which is its TARGET block, on its Mm rows: grid (blocks, P); rotation only
struct PopExplorePolicyArgs {
    const void *obs;          // [P][Mm][F], float32 or bfloat16, dense
    const float *agent_state; // [P][Mm][2]
    const float *target;      // [P][ExpNet::floats(F)]
    int8_t *rot;              // [P][Mm]
    int Mm, F, P;
};

// The acting kernels' grid rule per member (k_policy_flat's: a workgroup's two waves take a tile each), one round of
// resident workgroups shared among the members; *lds is the kernel's dynamic LDS
static inline int pop_policy_blocks(int Mm, int F, int P, size_t *lds)
{
    *lds = pol_flat_lds(F);
    int per_cu = (int)((160 * 1024) / *lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    const int ntiles = (Mm + 31) / 32;
    int blocks = (ntiles + 1) / 2;
    const int cap = (256 * per_cu + P - 1) / P;
    return blocks > cap ? cap : blocks;
}

// (the training step is ExpNet::launch_pop, antsrl_exptrain.h; a member's part of its workspace l1t_pop_stride<ExpNet>(B) bytes)
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_explore_policy(const PopExplorePolicyArgs &a, bool obs_bf16, hipStream_t st);

// ---- the population of joint agents (antsrl_popjoint.hip; include/antsrl.h, "The population of joint agents") ----
// A member's net is JointTrainer's flat block of JointNet::floats(F) floats (antsrl_jointtrain.h: w1 | b1 | w2 |
// b2 | w3 | b3): model, Adam's m and v and grads are [P][floats], the target's layer3 [P][99].  Blocks are 4-byte aligned
// and no more: every kernel reads and writes them float by float.

// the acting net of every member on its Mm rows: grid (blocks, P); layer1 and layer2 of the LIVE model block, layer3 of
// the target
struct PopJointPolicyArgs {
    const void *obs;          // [P][Mm][F], float32 or bfloat16, dense
    const float *agent_state; // [P][Mm][2]
    const float *model;       // [P][JointNet::floats(F)]
    const float *target_l3;   // [P][99]
    int8_t *rot, *ph;         // [P][Mm]
    int Mm, F, P;
};

// (the training step is JointNet::launch_pop, antsrl_jointtrain.h; a member's part of its workspace l1t_pop_stride<JointNet>(B) bytes)
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_joint_policy(const PopJointPolicyArgs &a, bool obs_bf16, hipStream_t st);

// ---- the population of memory nets (antsrl_popmemtrain.hip; include/antsrl.h, "The population of memory nets") ----
// A member's net is MemoryTrainer's state buffer (antsrl_memtrain.h: masters | m | v | packs): states and targets are
// [P][MemTrainLayout::bytes], the workspace [P][MemTrainWork::bytes], both strides multiples of 256 bytes (refused
// otherwise); grads [P][trained_floats], loss [P], idx [P][B] (required); the ring's arrays with a leading [P] of `rows`
// rows each, agent_states rows 2 + mem floats wide.  bt holds member 0's arrays; the table gives discount and step
// size, adam the common scalars.  17 launches: the single step's 16 of the grad stage and its apply, each on a grid (x, P).
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_memtrain(const MemNetDims &d, unsigned char *states, const unsigned char *targets,
                                                      const MemTrainBatch &bt, long long rows, int B, const PopTable &t, int P,
                                                      const AdamArgs &adam, float *grads, float *loss, const PopRunningLoss &rl,
                                                      unsigned char *work, hipStream_t st);

// The acting net of every member on its Mm rows (antsrl_popmemnet.hip): packs [P][pack_stride] bytes, a member's block
// antsrl_memnet_pack's; obs [P][Mm][F]; agent_state, mem_in, mem_out, rot, ph and q_out (or NULL) [P][Mm][...].  One
// launch on a grid (ceil(Mm / (32 nw)), P); member p's outputs are antsrl_launch_memnet's on its slice with its pack.
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_memnet(const unsigned char *packs, size_t pack_stride, const MemNetDims &d,
                                                    const void *obs, bool obs_bf16, const float *agent_state,
                                                    const float *mem_in, int Mm, int P, float *mem_out, int8_t *rot,
                                                    int8_t *ph, float *q_out, hipStream_t st);
// a: the single agent's SelArgs for member 0 WITH its memory part (mem_old, mem_next, env_elems, and mem_elems = member
// 0's elements; vec: they count float4).  The table gives seed and epsilon.  (antsrl_population.hip, beside k_pop_select)
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_memory_select(const SelArgs &a, const PopTable &t, int P, int Em, bool vec,
                                                           hipStream_t st);

// ---- the population of rework agents (antsrl_poprework.hip; include/antsrl.h, "The population of rework agents") ----
// A member's net is ReworkTrainer's flat block of NF = ReworkTrainLayout::off[20] floats (antsrl_reworktrain.h): model,
// target, Adam's m and v and grads are [P][NF]; a member's collapsed buffer (antsrl_rework.h) is CF = NQ D + NQ floats,
// collapsed [P][CF].  Neither count is a multiple of 4 in general (D = 296: CF = 1782), so blocks and buffers start
// 4-byte aligned and no more: every kernel reads and writes them one float at a time.

// tensor t of a member's block, the state_dict's order: what ReworkParams::p[t] is for a single net
struct PopReworkTensors {
    const float *block; // the member's
    const size_t *off;  // ReworkTrainLayout::off, where the kernel's arguments hold it
    __device__ __forceinline__ const float *operator[](int t) const { return block + off[t]; }
};

// the members' blocks for k_pop_rework_collapse: grid (NQ, P)
struct PopReworkCollapseArgs {
    const float *blocks; // [P][NF]
    float *collapsed;    // [P][CF]
    size_t off[2 * RW_LAYERS + 1]; // off[20] = NF
    ReworkDims d;
};

// the acting net of every member on its Mm rows: grid (blocks, P).  sel: member 0's (its seed and epsilon come from the
// table, env_base and explored move by Em); read by the SEL instantiations only
struct PopReworkActArgs {
    const float *collapsed;   // [P][CF]
    const void *obs;          // [P][Mm][F], float32 or bfloat16, dense; a member's slice a multiple of 16 bytes
    const float *agent_state; // [P][Mm][2]
    int8_t *rot, *ph;         // [P][Mm]
    float *q_out;             // [P][Mm][NQ] or NULL
    int Mm, Em, P;
    ReworkDims d;
    ReworkSelect sel;
};

// one launch each; `select`: act and epsilon-greedy in one (a.sel and the table's seeds and epsilons are read)
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_rework_collapse(const PopReworkCollapseArgs &a, int P, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_rework_act(const PopReworkActArgs &a, const PopTable &t, bool obs_bf16, bool select,
                                                        hipStream_t st);
// a: the single step's ReworkTrainArgs for member 0 (a.L antsrl_reworktrain_layout's for a.B; idx [P][B]; a.target the
// members' collapsed buffers); ws_stride: bytes between two members' parts of the workspace.  Four launches on grids
// (x, P); the table gives discount and step size
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_reworktrain(const ReworkTrainArgs &a, const PopTable &t, int P, size_t ws_stride,
                                                         const PopRunningLoss &rl, hipStream_t st);

// ---- population-based training (antsrl_popfitness.hip; include/antsrl.h, "Population-based training") ----
// row[p] = {total, min, max} of member p's environments [p Em, (p + 1) Em) of episode_reward (double [P Em][N], the
// monitor block's, read only): grid P, one workgroup of MON_THREADS = 256 per member.  THE ORDER OF THE SUMS is the
// monitor's (antsrl_monitor.h), every add a float64 add:
//     an environment's total:  the total[e] rule: slot t starts at +0.0 and adds ants t, t + 256, ... ascending; the 256
//                              slots are folded with x[i] += x[i + s] for i < s, s = 128, 64, ..., 1.
//     the member's total:      the same rule over its Em environment totals: slot t takes environments t, t + 256, ... of
//                              the member.
//     min / max:               of the environments' totals; order-free.
// (The exploit is antsrl_launch_env_copy's table, antsrl_checkpoint.h: no kernel of its own.)
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_fitness(const double *episode_reward, int Em, int N, int P, double *row, hipStream_t st);

// ---- the population of linear agents ----
// a: the single agent's SelArgs for member 0 (M = Mm); Em environments per member.  The table gives seed and epsilon.
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_policy(const PopPolicyArgs &a, bool obs_bf16, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_select(const SelArgs &a, const PopTable &t, int P, int Em, hipStream_t st);
// a: the single agent's RecArgs for member 0 (M = Mm, its K, the shared ring rows; memory NULL, or member 0's [Mm][mem]
// with mem > 0: the memory agents' ring); the table gives the seed
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_record(const RecArgs &a, const PopTable &t, int P, int Em, bool obs_bf16,
                                                    bool post, hipStream_t st);
// a: the single agent's LinTrainArgs for member 0 (B <= 512: one workgroup; idx [P][B]; adam.m of member 0, adam.v is
// adam.m + 198: a member's moments are [2][198]); the table gives discount and step size
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_lintrain(const LinTrainArgs &a, const PopTable &t, int P, const PopRunningLoss &rl,
                                                      hipStream_t st);
