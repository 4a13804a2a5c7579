// antsrl_dqn_dev.h — the device code the linear agent's training step (antsrl_lintrain.hip), the explore agent's
// (antsrl_exptrain.hip) and the joint step (antsrl_jointtrain.hip) share, once: the acting kernel's layer-1 sequence
// (k_policy_flat, antsrl_policy.hip) as the training forward restates it, the 3-output head, the tail of the epilogues
// and the layer1 stage of the two steps that train layer1 (the clamp that keeps idx inside the ring, dqn_row, is
// antsrl_dqn.h's: the rework agent's step takes it too).  Every helper is force-inlined and the build
// has -ffp-contract=off: a caller computes the bits it computed with the helper's body written out.
#pragma once
#include <hip/hip_runtime.h>
#include "antsrl_adam.h"
#include "antsrl_dqn.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
struct __attribute__((packed, aligned(4))) DqnF4 { float v[4]; }; // 4-byte aligned 16-byte load (rows with F % 4 != 0)

__device__ __forceinline__ void dqn_wave_sync()
{
    // LDS hand-off inside one wave: its LDS instructions execute in order, only the compiler must not reorder
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the observation columns of a W1 [32][F + 2] as the bf16 A operand w1s [32][KP] (zero for k >= F), by wave wib of nw
__device__ __forceinline__ void dqn_stage_w1(const float *__restrict__ w1, __bf16 *w1s, const int F, const int ksteps,
                                             const int KP, const int wib, const int nw, const int lane)
{
    for (int row = wib; row < DQN_HIDDEN; row += nw)
        for (int k = lane; k < 16 * ksteps; k += 64) {
            const float wv = w1[(size_t)row * (F + 2) + min(k, F - 1)];
            w1s[row * KP + k] = (__bf16)(k < F ? wv : 0.0f);
        }
}

// 8 consecutive inputs k0 .. k0 + 7 of a row as a bf16 fragment; inputs at or beyond F are zero and never read
__device__ __forceinline__ bf16x8 dqn_frag(const float *__restrict__ row, const int k0, const int F, const bool whole)
{
    bf16x8 b;
    if (whole) {
        const DqnF4 lo = *reinterpret_cast<const DqnF4 *>(row + k0), hi = *reinterpret_cast<const DqnF4 *>(row + k0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b[j] = (__bf16)lo.v[j];
            b[4 + j] = (__bf16)hi.v[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = row[min(k0 + j, F - 1)]; // unconditional on a clamped address, then a select
            b[j] = (__bf16)(k0 + j < F ? x : 0.0f);
        }
    }
    return b;
}

// a hidden value behind layer1's accumulator, k_policy_flat's expression: as0, as1 the bf16-rounded agent state, w0, w1
// the bf16-rounded W1 columns F, F + 1, b the fp32 bias
__device__ __forceinline__ float dqn_hidden(const float acc, const float as0, const float w0, const float as1,
                                            const float w1, const float b)
{
    return acc + (as0 * w0 + as1 * w1) + b;
}

// the three outputs of one head for this lane's row: the lane's 16 hidden values against its part of the weights, the
// other half-wave's part added, then the bias.  w: [3][32] + [3] in LDS
__device__ __forceinline__ void dqn_head(const float *w, const float (&hv)[16], const int h, float (&q)[3])
{
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        float p = 0.0f;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float4 ww = *reinterpret_cast<const float4 *>(w + o * DQN_HIDDEN + 8 * g4 + 4 * h);
            p += ww.x * hv[4 * g4];
            p += ww.y * hv[4 * g4 + 1];
            p += ww.z * hv[4 * g4 + 2];
            p += ww.w * hv[4 * g4 + 3];
        }
        q[o] = (p + __shfl_xor(p, 32)) + w[3 * DQN_HIDDEN + o];
    }
}

// the gradient of trained float i is `total`: stored (grads may be NULL), then Adam on that float
__device__ __forceinline__ void dqn_store_adam(float *params, float *grads, const AdamArgs &o, const size_t i,
                                               const float total)
{
    if (grads) grads[i] = total;
    if (o.on) adam_at(params, o, i, total);
}

// ---- the layer1 stage of a step that trains layer1 (k_exptrain_l1, antsrl_exptrain.hip; k_jointtrain_l1,
// antsrl_jointtrain.hip): one body, the net's flat block described by DqnL1Layout ------------------------------------------
#define DQN_L1_UNROLL 8 // rows per wave in flight

// where a flat block [w1 [32][F + 2] at 0 | ...] keeps what the stage writes, and what the forward stage left it
struct DqnL1Layout {
    size_t b1;    // offset of b1 [32]
    size_t heads; // offset of the floats behind layer1 whose gradients the forward stage's partials hold
    int nout;     // partial sums per workgroup of the forward stage: the heads' gradients in the block's order, then the loss
    int pitch;    // floats per row of the partials
};

__device__ __forceinline__ float dqn_bf16(const float x) { return (float)(__bf16)x; }

// columns k0 .. k0 + 3 of xe[b] = bf16(states[ri]) ++ bf16(agent_states[ri]) ++ 1 (zero beyond)
__device__ __forceinline__ void dqn_xe_cols(const DqnBatch &a, const long long ri, const int k0, float (&x)[4])
{
    const int F = a.F;
    if (k0 + 3 < F) {
        const DqnF4 v = *reinterpret_cast<const DqnF4 *>(a.states + (size_t)ri * F + k0);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = dqn_bf16(v.v[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + i;
            if (k < F) x[i] = dqn_bf16(a.states[(size_t)ri * F + k]);
            else if (k < F + 2) x[i] = dqn_bf16(a.agent_states[(size_t)ri * 2 + (k - F)]);
            else x[i] = k == F + 2 ? 1.0f : 0.0f;
        }
    }
}

// The body of a layer1 stage's kernel: 64 * DQN_L1_WAVES threads, nslabs + 1 workgroups, red [DQN_L1_WAVES * 32 *
// DQN_L1_SLAB] floats of LDS.  Workgroup s < nslabs owns columns 8 s .. 8 s + 7 of
//     g[j][k] = sum_b dh[b][j] * xe[b][k]       (columns 0 .. F + 1 are g_w1, column F + 2 is g_b1):
// lane (j, c) = (lane & 31, lane >> 5) of wave w keeps the four columns 8 s + 4 c .. + 3 of hidden unit j and walks rows
// w, w + 16, ... in ascending order, one fmaf per row and column from zero, DQN_L1_UNROLL rows' loads in flight; the 16
// waves' sums are added in wave order from wave 0's; the workgroup writes the gradient and runs Adam on its own columns.
// Workgroup nslabs adds the forward stage's partials in workgroup order, writes the heads' gradients and the loss and
// runs Adam on the heads.
__device__ __forceinline__ void dqn_l1_stage(const DqnBatch &mb, float *params, const AdamArgs &adam, const float *dh,
                                             const int blocks, const int nslabs, const DqnL1Layout lay, float *red)
{
    const int IN = mb.F + 2;
    if ((int)blockIdx.x == nslabs) { // the heads and the loss: the forward stage's partials in workgroup order
        if ((int)threadIdx.x >= lay.nout) return;
        float s = 0.0f;
        for (int b = 0; b < blocks; ++b) s += mb.partials[(size_t)b * lay.pitch + threadIdx.x];
        if ((int)threadIdx.x == lay.nout - 1) *mb.loss = s;
        else dqn_store_adam(params, mb.grads, adam, lay.heads + threadIdx.x, s);
        return;
    }
    const int lane = threadIdx.x & 63, j = lane & 31, c = lane >> 5, wib = threadIdx.x >> 6;
    const int k0 = blockIdx.x * DQN_L1_SLAB + 4 * c;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int b0 = wib; b0 < mb.B; b0 += DQN_L1_WAVES * DQN_L1_UNROLL) {
        float d[DQN_L1_UNROLL], x[DQN_L1_UNROLL][4];
#pragma unroll
        for (int u = 0; u < DQN_L1_UNROLL; ++u) { // the loads of DQN_L1_UNROLL rows first: they do not depend on one another
            const int b = min(b0 + DQN_L1_WAVES * u, mb.B - 1);
            d[u] = dh[(size_t)b * DQN_HIDDEN + j];
            dqn_xe_cols(mb, dqn_row(mb, b), k0, x[u]);
        }
#pragma unroll
        for (int u = 0; u < DQN_L1_UNROLL; ++u)
            if (b0 + DQN_L1_WAVES * u < mb.B) { // (uniform in the wave)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(d[u], x[u][i], acc[i]);
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(wib * DQN_HIDDEN + j) * DQN_L1_SLAB + 4 * c + i] = acc[i];
    __syncthreads();
    if (threadIdx.x >= DQN_HIDDEN * DQN_L1_SLAB) return;
    const int jj = threadIdx.x >> 3, col = threadIdx.x & 7, k = blockIdx.x * DQN_L1_SLAB + col;
    float s = red[jj * DQN_L1_SLAB + col];
#pragma unroll
    for (int w = 1; w < DQN_L1_WAVES; ++w) s += red[(w * DQN_HIDDEN + jj) * DQN_L1_SLAB + col];
    if (k < IN) dqn_store_adam(params, mb.grads, adam, (size_t)jj * IN + k, s);
    else if (k == IN) dqn_store_adam(params, mb.grads, adam, lay.b1 + jj, s);
}
