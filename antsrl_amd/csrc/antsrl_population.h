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
#include "antsrl_fail.h"
#include "antsrl_lintrain.h"
#include "antsrl_memagent.h"

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

// a: the single agent's SelArgs for member 0 (M = Mm); Em environments per member.  The table gives seed and epsilon.
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_policy(const PopPolicyArgs &a, bool obs_bf16, hipStream_t st);
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_select(const SelArgs &a, const PopTable &t, int P, int Em, hipStream_t st);
// a: the single agent's RecArgs for member 0 (M = Mm, its K, the shared ring rows); the table gives the seed
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_record(const RecArgs &a, const PopTable &t, int P, int Em, bool obs_bf16,
                                                    bool post, hipStream_t st);
// a: the single agent's LinTrainArgs for member 0 (B <= 512: one workgroup; idx [P][B]; adam.m of member 0, adam.v is
// adam.m + 198: a member's moments are [2][198]); the table gives discount and step size
ANTSRL_INTERNAL hipError_t antsrl_launch_pop_lintrain(const LinTrainArgs &a, const PopTable &t, int P, const PopRunningLoss &rl,
                                                      hipStream_t st);
