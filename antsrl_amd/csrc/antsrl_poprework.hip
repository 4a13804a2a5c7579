// antsrl_poprework.hip — P rework agents in lockstep on one handle (include/antsrl.h, "The population of rework agents";
// antsrl_population.h holds the layout; DESIGN.md §7.34 the reasons and the measurements): the collapse of every
// member's target net in one launch, the acting net with or without the epsilon-greedy select in one launch, and the
// training step in the single step's four launches, whatever P is.
//
// antsrl_population.hip's rule: each kernel is the single agent's stage with the member taken from blockIdx.y.  It
// moves the single agent's arguments (filled by the host for member 0) to its member and then runs the SAME body text
// the single agent's __global__ kernel runs, included inside both:
//   k_pop_rework_collapse                 antsrl_rework_collapse_body.inc    (k_rework_collapse)      grid (NQ, P)
//   k_pop_rework_act<OBS16, NQP, SEL>     antsrl_rework_act_body.inc         (k_rework_act)           grid (blocks, P)
//   k_pop_reworktrain_down                antsrl_reworktrain_down_body.inc   (k_reworktrain_down)     grid (NQ, P)
//   k_pop_reworktrain_batch<NQP>          antsrl_reworktrain_batch_body.inc  (k_reworktrain_batch)    grid (parts, P)
//   k_pop_reworktrain_up                  antsrl_reworktrain_up_body.inc     (k_reworktrain_up)       grid (NQ, P)
//   k_pop_reworktrain_grad                antsrl_reworktrain_grad_body.inc   (k_reworktrain_grad)     grid (ceil(NF / 256), P)
// A body reads the x dimension of the grid as its kernel always did.  So member p computes, bit for bit, what the single
// agent's kernels compute on its own block, collapsed buffer, rows, ring slab and part of the workspace: every order of
// sums is the single kernel's, and `parts` is the single step's for the same B, since the partials are added in
// workgroup order.  No atomics, no scratch; no kernel reads what another member's workgroups write.
//
// Alignment.  A member's block (NF floats) and collapsed buffer (CF = NQ D + NQ floats; D = 296 gives 1782) start 4-byte
// aligned and no more; every read and write of them, in the bodies and here, is one float at a time (the 16-byte reads
// are of LDS and of observation rows).  A member's observation rows start Mm F elements behind the previous member's:
// a multiple of 16 bytes by the entry's rule (pop_flat_rule's), so a member's first row starts as the single kernel
// expects its buffer to (4-byte aligned dwords on the bf16 path), and the bf16 path's last_dword is the member's own:
// no load of member p reaches into member p + 1's rows.  A member's part of the workspace starts a multiple of 256 bytes
// in, as a single step's workspace does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_draw.h"
#include "antsrl_lds_optin.h"
#include "antsrl_population_dev.h"

static_assert(RT_MAX_PARTS <= RT_TPB, "k_pop_reworktrain_up loads one partial per thread");
static_assert(sizeof(ReworkTrainArgs) + sizeof(PopTable) + sizeof(PopRunningLoss) + sizeof(size_t) <= 4096,
              "the training kernels' arguments");
static_assert(sizeof(PopReworkActArgs) + sizeof(PopTable) + sizeof(int) <= 4096, "k_pop_rework_act's arguments");

// ------------------------------------------------------------------ the collapse
__global__ void __launch_bounds__(RW_TPB) k_pop_rework_collapse(const PopReworkCollapseArgs pa)
{
    // the body's names, for this member: P.p[t] is tensor t of its block
    const size_t member = blockIdx.y;
    const ReworkDims &d = pa.d;
    const struct {
        PopReworkTensors p;
    } P = {{pa.blocks + member * pa.off[2 * RW_LAYERS], pa.off}};
    float *__restrict__ collapsed = pa.collapsed + member * ((size_t)(d.n_rot + d.n_ph) * (size_t)(d.D + 1));
#include "antsrl_rework_collapse_body.inc"
}

// ------------------------------------------------------------------ acting
// SEL false: antsrl_pop_policy_rework (`sel` and the table are not read); SEL true: antsrl_pop_policy_rework_select
template <bool OBS16, int NQP, bool SEL>
__global__ void __launch_bounds__(RW_TPB) k_pop_rework_act(const PopReworkActArgs pa, const PopTable tab, const int nchunks)
{
    // the body's names, for this member
    const size_t member = blockIdx.y, rows_m = (size_t)pa.Mm;
    const int M = pa.Mm, F = pa.d.F, n_rot = pa.d.n_rot, n_ph = pa.d.n_ph;
    const float *__restrict__ collapsed = pa.collapsed + member * ((size_t)(n_rot + n_ph) * (size_t)(pa.d.D + 1));
    const void *__restrict__ obs_ = reinterpret_cast<const unsigned char *>(pa.obs) + member * rows_m * (size_t)F * (OBS16 ? 2 : 4);
    const float *__restrict__ agent_state = pa.agent_state + member * rows_m * 2;
    int8_t *__restrict__ rot_out = pa.rot + member * rows_m, *__restrict__ ph_out = pa.ph + member * rows_m;
    float *__restrict__ q_out = pa.q_out ? pa.q_out + member * rows_m * (size_t)(n_rot + n_ph) : nullptr;
    ReworkSelect sel = pa.sel;
    if (SEL) {
        sel.seed = tab.m[member].seed;
        sel.epsilon = tab.m[member].epsilon;
        sel.env_base = pa.sel.env_base + (uint32_t)member * (uint32_t)pa.Em;
        sel.explored = pa.sel.explored ? pa.sel.explored + member * (size_t)pa.Em : nullptr;
    }
#include "antsrl_rework_act_body.inc"
}

// ------------------------------------------------------------------ training
__global__ void __launch_bounds__(RT_TPB) k_pop_reworktrain_down(const ReworkTrainArgs a0, const PopTable tab, const size_t ws_stride)
{
    const PopReworkTrainArgs a = pop_rt_member(a0, tab, blockIdx.y, ws_stride);
#include "antsrl_reworktrain_down_body.inc"
}

template <int NQP>
__global__ void __launch_bounds__(RT_TPB) k_pop_reworktrain_batch(const ReworkTrainArgs a0, const PopTable tab, const size_t ws_stride)
{
    const PopReworkTrainArgs a = pop_rt_member(a0, tab, blockIdx.y, ws_stride);
#include "antsrl_reworktrain_batch_body.inc"
}

// The member's running loss behind its up chain: main.py:106-109 in float64, antsrl_monitor.hip's arithmetic (each
// product rounded before the add: the build's -ffp-contract=off), by the thread that has just written the member's loss
// (thread RT_TPB - 65 of workgroup 0), as pop_l1t_l1_stage keeps it.
__global__ void __launch_bounds__(RT_TPB)
k_pop_reworktrain_up(const ReworkTrainArgs a0, const PopTable tab, const PopRunningLoss rl, const size_t ws_stride)
{
    const PopReworkTrainArgs a = pop_rt_member(a0, tab, blockIdx.y, ws_stride);
#include "antsrl_reworktrain_up_body.inc"
    if (rl.running_loss && blockIdx.x == 0 && threadIdx.x == RT_TPB - 65) {
        const double loss = (double)*a.loss;
        rl.running_loss[blockIdx.y] = rl.first ? loss : 0.99 * rl.running_loss[blockIdx.y] + 0.01 * loss;
    }
}

__global__ void __launch_bounds__(RT_TPB) k_pop_reworktrain_grad(const ReworkTrainArgs a0, const PopTable tab, const size_t ws_stride)
{
    const PopReworkTrainArgs a = pop_rt_member(a0, tab, blockIdx.y, ws_stride);
#include "antsrl_reworktrain_grad_body.inc"
}

// ------------------------------------------------------------------ launchers (antsrl_population.h)
hipError_t antsrl_launch_pop_rework_collapse(const PopReworkCollapseArgs &a, int P, hipStream_t st)
{
    if (P < 1 || P > ANTSRL_POP_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pop_rework_collapse, dim3((unsigned)(a.d.n_rot + a.d.n_ph), (unsigned)P), dim3(RW_TPB), 0, st, a);
    return hipGetLastError();
}

// k_rework_act's grid rule per member (a workgroup's four waves take 16 RW_U rows a pass), one round of RW_MAX_BLOCKS
// resident workgroups shared among the members, as pop_policy_blocks shares its round; rows beyond are looped.  The LDS
// opt-in is per kernel symbol, so every instantiation makes its own.
template <bool OBS16, int NQP, bool SEL>
static hipError_t pop_rw_launch_act(const PopReworkActArgs &a, const PopTable &t, hipStream_t st)
{
    const int nchunks = (a.d.D + 63) / 64;
    const size_t lds = (size_t)NQP * 64 * nchunks * sizeof(float); // <= 64 KiB (NQP 16, D 1024)
    const long long want = ((long long)a.Mm + 16 * RW_U - 1) / (16 * RW_U);
    const long long cap = (RW_MAX_BLOCKS + a.P - 1) / a.P;
    const int blocks = (int)(want < cap ? want : cap);
    const hipError_t e = antsrl_lds_optin<k_pop_rework_act<OBS16, NQP, SEL>>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_pop_rework_act<OBS16, NQP, SEL>), dim3((unsigned)blocks, (unsigned)a.P), dim3(RW_TPB), lds, st, a, t,
                       nchunks);
    return hipGetLastError();
}

template <bool OBS16, int NQP>
static hipError_t pop_rw_select_act(const PopReworkActArgs &a, const PopTable &t, bool select, hipStream_t st)
{
    return select ? pop_rw_launch_act<OBS16, NQP, true>(a, t, st) : pop_rw_launch_act<OBS16, NQP, false>(a, t, st);
}

hipError_t antsrl_launch_pop_rework_act(const PopReworkActArgs &a, const PopTable &t, bool obs_bf16, bool select, hipStream_t st)
{
    if (a.Mm < 1 || a.Em < 1 || a.P < 1 || a.P > ANTSRL_POP_MAX || a.d.D > RW_MAX_D) return hipErrorInvalidValue;
    const bool small = a.d.n_rot + a.d.n_ph <= 8;
    if (obs_bf16)
        return small ? pop_rw_select_act<true, 8>(a, t, select, st) : pop_rw_select_act<true, 16>(a, t, select, st);
    return small ? pop_rw_select_act<false, 8>(a, t, select, st) : pop_rw_select_act<false, 16>(a, t, select, st);
}

template <int NQP>
static hipError_t pop_rt_launch_batch(const ReworkTrainArgs &a, const PopTable &t, int P, size_t ws_stride, hipStream_t st)
{
    const int Dp = (a.d.D + 63) / 64 * 64;
    const size_t lds = sizeof(float) * ((size_t)2 * NQP * Dp + 2 * NQP + RT_ROWS * RT_INFO); // <= 128.6 KiB (NQP 16, D 1024)
    const hipError_t e = antsrl_lds_optin<k_pop_reworktrain_batch<NQP>>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_pop_reworktrain_batch<NQP>), dim3((unsigned)a.L.parts, (unsigned)P), dim3(RT_TPB), lds, st, a, t, ws_stride);
    return hipGetLastError();
}

hipError_t antsrl_launch_pop_reworktrain(const ReworkTrainArgs &a, const PopTable &t, int P, size_t ws_stride,
                                         const PopRunningLoss &rl, hipStream_t st)
{
    // the stride holds a member's part of the workspace and keeps every part 256-byte aligned
    if (P < 1 || P > ANTSRL_POP_MAX || ws_stride % 256 || ws_stride < a.L.bytes || a.L.parts < 1 || a.L.parts > RT_MAX_PARTS)
        return hipErrorInvalidValue;
    const int NQ = a.d.n_rot + a.d.n_ph;
    hipLaunchKernelGGL(k_pop_reworktrain_down, dim3((unsigned)NQ, (unsigned)P), dim3(RT_TPB), 0, st, a, t, ws_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = NQ <= 8 ? pop_rt_launch_batch<8>(a, t, P, ws_stride, st) : pop_rt_launch_batch<16>(a, t, P, ws_stride, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pop_reworktrain_up, dim3((unsigned)NQ, (unsigned)P), dim3(RT_TPB), 0, st, a, t, rl, ws_stride);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t NF = a.L.off[2 * RW_LAYERS];
    hipLaunchKernelGGL(k_pop_reworktrain_grad, dim3((unsigned)((NF + RT_TPB - 1) / RT_TPB), (unsigned)P), dim3(RT_TPB), 0, st, a, t,
                       ws_stride);
    return hipGetLastError();
}
