// antsrl_population.hip — P linear agents in lockstep on one handle, one launch per stage of the loop whatever P is
// (include/antsrl.h, "The population of linear agents"; antsrl_population.h holds the layout; DESIGN.md §7.24 the reasons
// and the measurements).
//
// Each kernel is the single agent's stage with the member taken from the grid.  It moves the single agent's arguments
// (filled by the host for member 0) to its member — pointers by the member's stride, the hyper-parameters from the
// by-value table — and then runs the SAME body text the single agent's __global__ kernel runs, included inside both:
//   k_pop_policy<OBS16>      antsrl_policy_flat_body.inc       (k_policy_flat)      grid (blocks, P)
//   k_pop_select             antsrl_agent_select_actions.inc   (k_agent_select)     grid (blocks, P)
//   k_pop_memory_select<V>   ... and antsrl_agent_select_memory.inc (k_agent_select)    grid (blocks, P)
//   k_pop_record<BF16, POST> antsrl_replay_record_body.inc     (k_replay_record)    grid (ceil(K / 4), P)
//   k_pop_lintrain           antsrl_lintrain_body.inc, NW = 4  (k_lintrain<4>)      grid (1, P)
// A body reads the x dimension of the grid as its kernel always did; the member is the y dimension.  The bodies are
// textual includes, not __device__ functions: a callee is optimised on its own before it is inlined, and the single
// agent's kernels then compiled to other code than they had; included, they compile to exactly what they were (§7.24).
// So member p computes, bit for bit, what the single agent's kernels compute on a handle of its Em environments created
// with env_id_base + p Em: the bodies see nothing but their own member's rows, and every draw is keyed on the global
// environment id.  No atomics; no kernel reads what another member's workgroups write.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_lintrain_dev.h"
#include "antsrl_memagent_dev.h"
#include "antsrl_population_dev.h"

// the table is a kernel argument of three kernels, beside the single agent's argument struct
static_assert(sizeof(PopTable) + sizeof(LinTrainArgs) + sizeof(PopRunningLoss) <= 4096, "k_pop_lintrain's arguments");
static_assert(sizeof(PopTable) + sizeof(SelArgs) + sizeof(uint32_t) <= 4096, "k_pop_select's arguments");
static_assert(sizeof(PopTable) + sizeof(RecArgs) + sizeof(uint32_t) <= 4096, "k_pop_record's arguments");

// ------------------------------------------------------------------ acting
// A workgroup stages ITS member's W1 in LDS and loops over that member's tiles only (blockIdx.y is the member).  The
// member's rows start Mm * F elements behind the previous member's: 16-byte aligned by the entry's alignment rule.
template <bool OBS16>
__global__ void __launch_bounds__(POL_FLAT_THREADS)
k_pop_policy(const PopPolicyArgs pa, const int ksteps, const int tile_elems)
{
    // the body's names, for this member
    const size_t member = blockIdx.y, rows_m = (size_t)pa.Mm, in_m = (size_t)pa.F + 2;
    const float *__restrict__ obs = reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(pa.obs) +
                                                                     member * rows_m * (size_t)pa.F * (OBS16 ? 2 : 4));
    const float *__restrict__ agent_state = pa.agent_state + member * rows_m * 2;
    const float *__restrict__ w1 = pa.w1 + member * LT_HIDDEN * in_m, *__restrict__ b1 = pa.b1 + member * LT_HIDDEN;
    // the acting net is the target net (collect_agent.py:166): the shared layer1, the live layer2, the target's layer3
    const float *__restrict__ w2 = pa.heads + member * LT_HEADS, *__restrict__ b2 = w2 + 96;
    const float *__restrict__ w3 = pa.target_l3 + member * LT_L3, *__restrict__ b3 = w3 + 96;
    int8_t *__restrict__ rot_out = pa.rot + member * rows_m, *__restrict__ ph_out = pa.ph + member * rows_m;
    float *__restrict__ logits_out = nullptr;
    const int M = pa.Mm, F = pa.F;
#include "antsrl_policy_flat_body.inc"
}

// ------------------------------------------------------------------ epsilon-greedy
__device__ __forceinline__ SelArgs pop_select_member(const SelArgs &a0, const PopTable &tab, const uint32_t member, const uint32_t Em)
{
    SelArgs a = a0;
    a.seed = tab.m[member].seed;
    a.epsilon = tab.m[member].epsilon;
    a.env_base = a0.env_base + member * Em;
    a.rot = a0.rot + (size_t)member * a0.M;
    a.ph = a0.ph + (size_t)member * a0.M;
    a.explored = a0.explored ? a0.explored + (size_t)member * Em : nullptr;
    return a;
}

__global__ __launch_bounds__(256) void k_pop_select(const SelArgs a0, const PopTable tab, const uint32_t Em)
{
    const SelArgs a = pop_select_member(a0, tab, blockIdx.y, Em);
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nthr = (uint64_t)gridDim.x * 256;
#include "antsrl_agent_select_actions.inc"
}

// The select of a population of memory agents: k_agent_select's two parts for its member.  a0.mem_elems counts MEMBER 0's
// memory elements in V units (V = 4: float4), so the member's halves start member * mem_elems * V floats on; both texts
// then see nothing but their member's ants and environments.
template <int V>
__global__ __launch_bounds__(256) void k_pop_memory_select(const SelArgs a0, const PopTable tab, const uint32_t Em)
{
    SelArgs a = pop_select_member(a0, tab, blockIdx.y, Em);
    a.mem_old = a0.mem_old + (size_t)blockIdx.y * a0.mem_elems * V;
    a.mem_next = a0.mem_next + (size_t)blockIdx.y * a0.mem_elems * V;
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nthr = (uint64_t)gridDim.x * 256;
#include "antsrl_agent_select_actions.inc"
#include "antsrl_agent_select_memory.inc"
}

// ------------------------------------------------------------------ the ring
template <bool BF16, bool POST>
__device__ __forceinline__ RecArgs pop_record_member(const RecArgs &a0, const PopTable &tab, const size_t member, const uint32_t Em)
{
    const size_t Mm = (size_t)a0.M, L = (size_t)a0.max_len;
    RecArgs a = a0;
    a.seed = tab.m[member].seed;
    a.env_base = a0.env_base + member * Em;
    a.obs = reinterpret_cast<const unsigned char *>(a0.obs) + member * Mm * (size_t)a0.pitch * (BF16 ? 2 : 4);
    a.agent_state = a0.agent_state + member * Mm * (size_t)a0.A;
    a.memory = a0.memory ? a0.memory + member * Mm * (size_t)a0.mem : nullptr; // (the memory agents' ring: mem > 0)
    a.states = a0.states + member * L * (size_t)a0.F;
    a.agent_states = a0.agent_states + member * L * (size_t)(a0.A + a0.mem);
    if (POST) {
        a.reward = a0.reward + member * Mm;
        a.done = a0.done + member * Em;
        a.rewards = a0.rewards + member * L;
        a.dones = a0.dones + member * L;
    } else {
        a.rot = a0.rot + member * Mm;
        a.ph = a0.ph ? a0.ph + member * Mm : nullptr;
        a.actions = a0.actions + member * L * 2;
    }
    return a;
}

template <bool BF16, bool POST>
__global__ __launch_bounds__(256) void k_pop_record(const RecArgs a0, const PopTable tab, const uint32_t Em)
{
    const RecArgs a = pop_record_member<BF16, POST>(a0, tab, blockIdx.y, Em);
#include "antsrl_replay_record_body.inc"
}

// ------------------------------------------------------------------ training
__device__ __forceinline__ LinTrainArgs pop_lintrain_member(const LinTrainArgs &a0, const PopTable &tab, const size_t member)
{
    const size_t L = (size_t)a0.batch.n_rows, F = (size_t)a0.batch.F;
    LinTrainArgs a = a0;
    a.w1 = a0.w1 + member * LT_HIDDEN * (F + 2);
    a.b1 = a0.b1 + member * LT_HIDDEN;
    a.heads = a0.heads + member * LT_HEADS;
    a.target_l3 = a0.target_l3 + member * LT_L3;
    a.adam.m = a0.adam.m + member * 2 * LT_HEADS;
    a.adam.v = a0.adam.v + member * 2 * LT_HEADS;
    a.adam.step_size = tab.m[member].step_size;
    pop_ring_member(a.batch, a0.batch, member, L, F);
    a.batch.grads = a0.batch.grads ? a0.batch.grads + member * LT_HEADS : nullptr;
    a.batch.loss = a0.batch.loss + member;
    a.batch.discount = tab.m[member].discount;
    return a;
}

// One workgroup per member (grid (1, P): gridDim.x == 1 is the body's fused form), each k_lintrain<4>'s one-workgroup
// step (B <= 512) on its member's net, Adam moments and ring slab, with the member's discount and Adam step size.
// One wave per SIMD (amdgpu_waves_per_eu(1, 1)) and the LDS opt-in, as k_lintrain: DESIGN §7.13 records a one-in-seventeen
// difference of one workgroup's partials when two such workgroups shared a CU (mechanism unknown), and none in 400
// launches with one wave per SIMD.  A population launches P <= ANTSRL_POP_MAX = 64 workgroups of four waves on 256 CUs,
// every one alone on its CU: inside the regime that note found clean.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_pop_lintrain(const LinTrainArgs a0, const PopTable tab, const PopRunningLoss rl)
{
    const LinTrainArgs a = pop_lintrain_member(a0, tab, blockIdx.y);
    constexpr int NW = 4;
#include "antsrl_lintrain_body.inc"
    // main.py:106-109 in float64, antsrl_monitor.hip's arithmetic (each product rounded before the add: the build's
    // -ffp-contract=off), by the thread that has just written the member's loss.  (pop_l1t_l1_stage has the same four
    // lines: called from one helper, this kernel's code differs)
    if (rl.running_loss && threadIdx.x == LT_HEADS) {
        const double l = (double)*a.batch.loss;
        rl.running_loss[blockIdx.y] = rl.first ? l : 0.99 * rl.running_loss[blockIdx.y] + 0.01 * l;
    }
}

// ------------------------------------------------------------------ launchers (antsrl_population.h)
hipError_t antsrl_launch_pop_policy(const PopPolicyArgs &a, bool obs_bf16, hipStream_t st)
{
    return pop_policy_launch<k_pop_policy<true>, k_pop_policy<false>>(a, obs_bf16, st);
}

hipError_t antsrl_launch_pop_select(const SelArgs &a, const PopTable &t, int P, int Em, hipStream_t st)
{
    hipLaunchKernelGGL(k_pop_select, dim3(grid_for((size_t)a.M), (unsigned)P), dim3(256), 0, st, a, t, (uint32_t)Em);
    return hipGetLastError();
}

hipError_t antsrl_launch_pop_memory_select(const SelArgs &a, const PopTable &t, int P, int Em, bool vec, hipStream_t st)
{
    // antsrl_launch_agent_select's grid for one member, a row of it per member
    const uint64_t work = a.mem_old == a.mem_next ? a.M : (a.mem_elems > a.M ? a.mem_elems : a.M);
    const dim3 grid(grid_for((size_t)work), (unsigned)P);
    if (vec)
        hipLaunchKernelGGL(k_pop_memory_select<4>, grid, dim3(256), 0, st, a, t, (uint32_t)Em);
    else
        hipLaunchKernelGGL(k_pop_memory_select<1>, grid, dim3(256), 0, st, a, t, (uint32_t)Em);
    return hipGetLastError();
}

hipError_t antsrl_launch_pop_record(const RecArgs &a, const PopTable &t, int P, int Em, bool obs_bf16, bool post, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n_write + 3) / 4), (unsigned)P), block(256);
    if (!post && obs_bf16)
        hipLaunchKernelGGL((k_pop_record<true, false>), grid, block, 0, st, a, t, (uint32_t)Em);
    else if (!post)
        hipLaunchKernelGGL((k_pop_record<false, false>), grid, block, 0, st, a, t, (uint32_t)Em);
    else if (obs_bf16)
        hipLaunchKernelGGL((k_pop_record<true, true>), grid, block, 0, st, a, t, (uint32_t)Em);
    else
        hipLaunchKernelGGL((k_pop_record<false, true>), grid, block, 0, st, a, t, (uint32_t)Em);
    return hipGetLastError();
}

hipError_t antsrl_launch_pop_lintrain(const LinTrainArgs &a, const PopTable &t, int P, const PopRunningLoss &rl, hipStream_t st)
{
    if (a.batch.ntiles > LT_FUSED_TILES) return hipErrorInvalidValue; // (the entry refuses B > 512 in words)
    const size_t lds = lt_lds(a.batch.ksteps, 4);
    const hipError_t e = antsrl_lds_optin<k_pop_lintrain>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pop_lintrain, dim3(1, (unsigned)P), dim3(256), lds, st, a, t, rl);
    return hipGetLastError();
}
