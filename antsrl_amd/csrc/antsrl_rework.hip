// antsrl_rework.hip — inference of the rework agent's net (CollectModelRework, agents/collect_agent_rework.py:24-63;
// antsrl_rework.h has the shapes and the collapsed buffer): the ten layers have no activation between them, so they are
// multiplied out once per weight change (k_rework_collapse, float64) and every step is NQ dot products of length D per
// row (k_rework_act, fp32): a stream over the observation tensor.
//
// k_rework_collapse — one workgroup per output row o of Wc (NQ workgroups of 256 threads).  Row o of the head's last layer
// (rotation_layer4 row o for o < n_rot, else pheromone_layer2 row o - n_rot) is widened to float64 as v, bc = that
// layer's bias[o]; then v is pushed down through the layers below it, the head's own first and layer4, 3, 2, 1 last
// (W_l [out][in], b_l [out], float32 widened exactly):
//     bc  <- (((bc + v[0] b_l[0]) + v[1] b_l[1]) + ...) + v[out-1] b_l[out-1]
//     v'[c] = (((0 + v[0] W_l[0][c]) + v[1] W_l[1][c]) + ...) + v[out-1] W_l[out-1][c]        for every c < in
// every product rounded to float64 before it is added (-ffp-contract=off), the contracted index ascending: thread t
// owns the columns c = t, t + 256, ... (coalesced over W_l's rows), the last thread also the bias sum.  v lives in
// LDS (two buffers of RW_MAX_D doubles).  After layer1, Wc[o][c] = (float)v[c] and bc[o] = (float)bc: one rounding
// each.  No atomics: every launch gives the same bits.  It runs once per weight change and is not tuned.
//
// k_rework_act<OBS16, NQP, SEL = false> — q[m][o] = bc[o] + sum_k x[m][k] Wc[o][k], x = cat[obs row, agent_state row], both argmaxes
// (first maximum).  NQP is NQ padded to 8 or 16 (zero rows), so that the accumulators stay in registers.  Wc is copied
// once per workgroup into LDS (NQP x Dp floats, Dp = D rounded up to 64, zero beyond D, in the order the lanes read it).
// Sixteen lanes share a row: lane l of the group takes k = 64 c + 4 l .. + 3 of every 64-input chunk c, so a group reads
// 256 contiguous bytes (fp32) of its row per load instruction and a wave four rows; a wave works on two such sets of
// four rows at a time (RW_U) and issues the loads of four chunks together (RW_G).  Outputs 2 p and 2 p + 1 share one
// packed fma (v_pk_fma_f32: each half is the fmaf below).
// Order of a row's sums, the same for every row whatever M, its place in the batch, the grid and the format:
//     lane l:   a = 0;  for c ascending, for i = 0..3:  a = fmaf(x[64 c + 4 l + i], Wc[o][64 c + 4 l + i], a)
//     group:    a += a of lane l ^ 1;  then l ^ 2;  then 7 - l within its eight;  then 15 - l     (every lane holds the sum)
//     q = a + bc[o]
// Loads: a chunk that lies inside the observation row (64 (c + 1) <= F) is read with one 16-byte load per lane (fp32,
// 4-byte aligned: a row starts at 4 m F bytes) or three aligned dwords and a funnel shift (bf16: a row starts at 2 m F
// bytes, on an odd element for odd m F; the third dword is clamped to the buffer's last whole dword and is only used
// where it lies inside).  The chunks that hold the row's end, the two agent_state inputs and the zero pad are read
// element by element on addresses clamped into the row, then selected.  Rows past M are clamped to row M - 1 and not
// written.  Nothing outside obs, agent_state and the collapsed buffer is read.
//
// k_rework_act<OBS16, NQP, SEL = true>, "k_rework_act_select" — k_rework_act and antsrl_agent_select_actions'
// epsilon-greedy in one launch (antsrl_policy_rework_select).  It is the same kernel text, so an evaluated row gets
// k_rework_act's bits, and SEL = false compiles to the instructions and registers it had without the switch.  A wave pass is
// 4 RW_U consecutive rows, hence a contiguous range of colonies.  In front of its loads the pass finds out which of its
// rows belong to a colony that explores this step (antsrl_draw.h): lane j of the wave looks after row j of the pass.
// When the pass lies inside one colony (always, once n_ants is a multiple of 4 RW_U) the colony and its explore draw are
// wave-uniform and computed once, in scalar registers; a pass that straddles colonies makes one draw per row and
// collects the flags with a ballot.  Either way the flags end up in a scalar mask and every branch on it is wave-uniform:
//     every row of the pass explores:  no load, no fma; lanes 0 .. 4 RW_U - 1 draw their row's two actions and store them
//     no row explores:                 k_rework_act's pass
//     mixed:                           the exploring rows' lanes draw and store, then k_rework_act's pass on all rows,
//                                      of which the evaluating lanes of the exploring rows store nothing (actions or q)
// The three draws of a row share their first two rounds (draw_env_step: colony and step); a drawn action costs the other
// two.  explored[e] is written by the lane whose row is colony e's first ant: one writer.  No atomics, no LDS beyond Wc.
//
// Both bodies are textual includes (antsrl_rework_collapse_body.inc, antsrl_rework_act_body.inc): the population's
// kernels (antsrl_poprework.hip) run the same text on a member's block and rows, and these two compile to what they
// compiled to with the text in place.  The launch constants and rw_in are antsrl_rework.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_draw.h"
#include "antsrl_rework.h"

__global__ void __launch_bounds__(RW_TPB)
k_rework_collapse(const ReworkParams P, const ReworkDims d, float *__restrict__ collapsed)
{
#include "antsrl_rework_collapse_body.inc"
}

hipError_t antsrl_launch_rework_collapse(const ReworkParams &P, const ReworkDims &d, float *collapsed, hipStream_t st)
{
    hipLaunchKernelGGL(k_rework_collapse, dim3(d.n_rot + d.n_ph), dim3(RW_TPB), 0, st, P, d, collapsed);
    return hipGetLastError();
}

// SEL false: antsrl_policy_rework (`sel` is not read); SEL true: antsrl_policy_rework_select ("k_rework_act_select")
template <bool OBS16, int NQP, bool SEL>
__global__ void __launch_bounds__(RW_TPB)
k_rework_act(const float *__restrict__ collapsed, const void *__restrict__ obs_, const float *__restrict__ agent_state,
             int8_t *__restrict__ rot_out, int8_t *__restrict__ ph_out, float *__restrict__ q_out, const int M, const int F,
             const int n_rot, const int n_ph, const int nchunks, const ReworkSelect sel)
{
#include "antsrl_rework_act_body.inc"
}

// sel: NULL launches k_rework_act
template <bool OBS16, int NQP>
static hipError_t rw_launch_act(const float *collapsed, const ReworkDims &d, const void *obs, const float *agent_state, int M,
                                const ReworkSelect *sel, int8_t *rot, int8_t *ph, float *q_out, hipStream_t st)
{
    const int nchunks = (d.D + 63) / 64;
    const size_t lds = (size_t)NQP * 64 * nchunks * sizeof(float); // <= 64 KiB (NQP 16, D 1024)
    const long long want = ((long long)M + 16 * RW_U - 1) / (16 * RW_U); // a workgroup's four waves take 16 RW_U rows a pass
    const int blocks = (int)(want < RW_MAX_BLOCKS ? want : RW_MAX_BLOCKS);
    if (sel)
        hipLaunchKernelGGL((k_rework_act<OBS16, NQP, true>), dim3(blocks), dim3(RW_TPB), lds, st, collapsed, obs, agent_state,
                           rot, ph, q_out, M, d.F, d.n_rot, d.n_ph, nchunks, *sel);
    else
        hipLaunchKernelGGL((k_rework_act<OBS16, NQP, false>), dim3(blocks), dim3(RW_TPB), lds, st, collapsed, obs, agent_state,
                           rot, ph, q_out, M, d.F, d.n_rot, d.n_ph, nchunks, ReworkSelect{});
    return hipGetLastError();
}

static hipError_t rw_dispatch_act(const float *collapsed, const ReworkDims &d, const void *obs, bool obs_bf16,
                                  const float *agent_state, int M, const ReworkSelect *sel, int8_t *rot, int8_t *ph,
                                  float *q_out, hipStream_t st)
{
    const bool small = d.n_rot + d.n_ph <= 8;
    if (obs_bf16)
        return small ? rw_launch_act<true, 8>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st)
                     : rw_launch_act<true, 16>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st);
    return small ? rw_launch_act<false, 8>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st)
                 : rw_launch_act<false, 16>(collapsed, d, obs, agent_state, M, sel, rot, ph, q_out, st);
}

hipError_t antsrl_launch_rework_act(const float *collapsed, const ReworkDims &d, const void *obs, bool obs_bf16,
                                    const float *agent_state, int M, int8_t *rot, int8_t *ph, float *q_out, hipStream_t st)
{
    return rw_dispatch_act(collapsed, d, obs, obs_bf16, agent_state, M, nullptr, rot, ph, q_out, st);
}

hipError_t antsrl_launch_rework_act_select(const float *collapsed, const ReworkDims &d, const void *obs, bool obs_bf16,
                                           const float *agent_state, int M, const ReworkSelect &sel, int8_t *rot, int8_t *ph,
                                           float *q_out, hipStream_t st)
{
    return rw_dispatch_act(collapsed, d, obs, obs_bf16, agent_state, M, &sel, rot, ph, q_out, st);
}
