// antsrl_dqn_dev.h — the device code the linear agent's training step (antsrl_lintrain.hip) and the explore agent's
// (antsrl_exptrain.hip) share, once: the acting kernel's layer-1 sequence (k_policy_flat, antsrl_policy.hip) as the
// training forward restates it, the 3-output head and the tail of the epilogues (the clamp that keeps idx inside the
// ring, dqn_row, is antsrl_dqn.h's: the rework agent's step takes it too).  Every helper is force-inlined and the build
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
