// antsrl_reworktrain.hip — the DQN training step of the rework agent's net (CollectAgentRework.train,
// agents/collect_agent_rework.py:110-152; antsrl_reworktrain.h has the arguments and the workspace's layout,
// include/antsrl.h the contract).  CollectModelRework has no activation, so with x[b] a minibatch row, dq[b] the loss's
// derivative by the row's NQ outputs (non-zero at the two actions taken only),
//     G = sum_b dq[b] (x) x[b]  [NQ][D],   s = sum_b dq[b]  [NQ]
// M_l [NQ][out_l] the head rows pushed DOWN to layer l's output (the v of k_rework_collapse on its way; the unit rows at a
// head's last layer) and A_l [NQ][out_l] the pseudo-rows pushed UP (A_l = A_in(l) W_l^T + s (x) b_l, A of x being G), every
// layer's gradient is
//     dW_l = sum_k M_l[k] (x) A_in(l)[k],   db_l = sum_k M_l[k] s[k]        k over the pseudo-rows of l's head
// and no B x width activation exists.  Four launches, no atomics, every sum in a fixed order:
//
// k_reworktrain_down  — k_rework_collapse on the flat block (one workgroup per row o, the same float64 sequence, so the
//     model's collapsed buffer has that kernel's bits), storing v in front of every push as M_l[o]; rows of the other
//     head's layers are written as zeros.
// k_reworktrain_batch<NQP> — the stream over the rows: the hot path.  Both collapsed buffers (the model's from the
//     workspace, the target's from the caller) lie in LDS, zero-padded to [NQP][Dp], Dp = D rounded up to 64.  A workgroup
//     takes RT_ROWS = 16 minibatch rows at a time, one per 16 lanes, in k_rework_act's lane layout and order of sums
//     (lane l: k = 64 c + 4 l .. + 3, c ascending, fmaf; the group sum by DPP; + bc): q of the row under the model, q' of
//     its successor under the target, then per head
//         y = reward + discount * max q' * !done,   d = q[a] - y,   g = d * 2 / (n B)
//     (a clamped to [0, n)), handed over in LDS.  Then thread t owns the columns c = t, t + 256, ... of G: for the 16 rows
//     in ascending order it reads x[c] again (the line is in cache) and adds g_rot x[c] to its accumulator of row a_rot and
//     g_ph x[c] to that of row n_rot + a_ph: product rounded, then added; NQP accumulators per column, selected, not
//     indexed.  s and the two sums of d^2 ride along in threads 0 .. NQ - 1 and 64.  Rows beyond the grid's reach are
//     looped (workgroup w: rows 16 (w + i parts) ..), so a workgroup's partial is a sum over its rows in ascending order
//     from zero; it is written to slot w of the workspace.  Rows past B are row B - 1 with g = 0.
//     Loads: a chunk inside the observation row with one 4-byte-aligned 16-byte load per lane, the chunk with the row's
//     end, agent_state and the pad element by element on addresses clamped into the row, then selected.  idx is clamped
//     to [0, n_rows).  Nothing outside the arrays is read.
// k_reworktrain_up    — one workgroup per pseudo-row k: the partials added in workgroup order from zero (fp32) give
//     G[k], s[k] and, in workgroup 0, loss = L_rot / (n_rot B) + L_ph / (n_ph B); then A_l[k] in float64, thread j the
//     output j:  a = ((0 + A_in[0] W[j][0]) + A_in[1] W[j][1]) + ..., then a + s[k] b[j]; every product rounded before it is
//     added.  layer1..4, then rotation_layer1..3 (k < n_rot) or pheromone_layer1 (the others' rows: zeros).
// k_reworktrain_grad  — one thread per trained float i: its tensor from the block's offsets, then
//     (float)(((0 + M_l[k0][o] A[k0][c]) + M_l[k0 + 1][o] A[k0 + 1][c]) + ...) in float64 (s[k] for a bias, G widened for
//     layer1), stored if the caller wants it, and Adam on that float (adam_at) in a fused step.
//
// The four bodies are textual includes (antsrl_reworktrain_down / _batch / _up / _grad_body.inc): the population's
// kernels (antsrl_poprework.hip) run the same text on a member's arguments, and these four compile to what they compiled
// to with the text in place.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_lds_optin.h"
#include "antsrl_reworktrain.h"

static_assert(RT_MAX_PARTS <= RT_TPB, "k_reworktrain_up loads one partial per thread");

void antsrl_reworktrain_layout(const ReworkDims &d, int B, ReworkTrainLayout *L)
{
    const int NQ = d.n_rot + d.n_ph;
    const int out[RW_LAYERS] = {d.g1, d.g2, d.g3, d.D, d.r1, d.r2, d.r3, d.n_rot, d.p1, d.n_ph};
    const int in[RW_LAYERS] = {d.D, d.g1, d.g2, d.g3, d.D, d.r1, d.r2, d.r3, d.D, d.p1};
    const int src[RW_LAYERS] = {-1, 0, 1, 2, 3, 4, 5, 6, 3, 8};
    size_t off = 0;
    for (int l = 0; l < RW_LAYERS; ++l) {
        L->out[l] = out[l];
        L->in[l] = in[l];
        L->src[l] = src[l];
        L->k0[l] = l < 4 ? 0 : (l < 8 ? 0 : d.n_rot);
        L->k1[l] = l < 4 ? NQ : (l < 8 ? d.n_rot : NQ);
        L->off[2 * l] = off;
        off += (size_t)out[l] * in[l];
        L->off[2 * l + 1] = off;
        off += (size_t)out[l];
    }
    L->off[2 * RW_LAYERS] = off;
    const int passes = (B + RT_ROWS - 1) / RT_ROWS;
    L->parts = passes < RT_MAX_PARTS ? passes : RT_MAX_PARTS;
    L->part_stride = (NQ * d.D + NQ + 2 + 63) / 64 * 64;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    L->collapsed = take(sizeof(float) * ((size_t)NQ * d.D + NQ));
    for (int l = 0; l < RW_LAYERS; ++l) L->M[l] = take(sizeof(double) * NQ * out[l]);
    L->partials = take(sizeof(float) * (size_t)L->parts * L->part_stride);
    L->G = take(sizeof(float) * ((size_t)NQ * d.D + NQ));
    for (int l = 0; l < RW_LAYERS; ++l) L->A[l] = (l == 7 || l == 9) ? 0 : take(sizeof(double) * NQ * out[l]);
    L->bytes = at;
}

__global__ void __launch_bounds__(RT_TPB) k_reworktrain_down(const ReworkTrainArgs a)
{
#include "antsrl_reworktrain_down_body.inc"
}

template <int NQP>
__global__ void __launch_bounds__(RT_TPB) k_reworktrain_batch(const ReworkTrainArgs a)
{
#include "antsrl_reworktrain_batch_body.inc"
}

__global__ void __launch_bounds__(RT_TPB) k_reworktrain_up(const ReworkTrainArgs a)
{
#include "antsrl_reworktrain_up_body.inc"
}

__global__ void __launch_bounds__(RT_TPB) k_reworktrain_grad(const ReworkTrainArgs a)
{
#include "antsrl_reworktrain_grad_body.inc"
}

template <int NQP>
static hipError_t rt_launch_batch(const ReworkTrainArgs &a, hipStream_t st)
{
    const int Dp = (a.d.D + 63) / 64 * 64;
    const size_t lds = sizeof(float) * ((size_t)2 * NQP * Dp + 2 * NQP + RT_ROWS * RT_INFO); // <= 128.6 KiB (NQP 16, D 1024)
    if (lds > 65536) {
        const hipError_t e = antsrl_lds_optin<k_reworktrain_batch<NQP>>(lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_reworktrain_batch<NQP>), dim3(a.L.parts), dim3(RT_TPB), lds, st, a);
    return hipGetLastError();
}

hipError_t antsrl_launch_reworktrain(const ReworkTrainArgs &a, hipStream_t st)
{
    const int NQ = a.d.n_rot + a.d.n_ph;
    hipLaunchKernelGGL(k_reworktrain_down, dim3(NQ), dim3(RT_TPB), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = NQ <= 8 ? rt_launch_batch<8>(a, st) : rt_launch_batch<16>(a, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_reworktrain_up, dim3(NQ), dim3(RT_TPB), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t P = a.L.off[2 * RW_LAYERS];
    hipLaunchKernelGGL(k_reworktrain_grad, dim3((unsigned)((P + RT_TPB - 1) / RT_TPB)), dim3(RT_TPB), 0, st, a);
    return hipGetLastError();
}
