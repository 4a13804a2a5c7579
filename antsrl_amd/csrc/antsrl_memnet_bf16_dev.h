// antsrl_memnet_bf16_dev.h — the device helpers of the bf16 forward of the memory agent's net, for the two kernels that
// run its body text (antsrl_memnet_body.inc): k_memnet (antsrl_memnet.hip) and k_pop_memnet (antsrl_popmemnet.hip).
// The staging of a weight chunk, the two tile products, the two whole-layer walks and the workgroup's constants.  These
// were __forceinline__ functions of antsrl_memnet.hip and are the same text here; the steps inside the kernel stay in
// the body text (antsrl_memnet_dev.h says why they are not functions).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_memnet.h"
#include "antsrl_memnet_dev.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

#define MN_MAXT 8 // hidden tiles held in registers: widths <= 256

__device__ __forceinline__ void mn_to_b(const f32x16 &v, bf16x8 &b0, bf16x8 &b1)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        b0[j] = (__bf16)v[j];
        b1[j] = (__bf16)v[8 + j];
    }
}

#ifndef MN_SBATCH
#define MN_SBATCH 8 // 16-byte loads in flight per thread while a weight chunk is staged
#endif

// The workgroup's waves (each with its own 32 ants) walk the same sequence of layers and output tiles, so every A
// fragment is fetched from global memory ONCE per workgroup: mn_stage copies the fragments of the next whole output
// tiles of a layer (as many as fit in `wcap` 16-byte units) into the shared LDS buffer, between two barriers, and
// returns tile t's fragments there.  All waves call it at the same points (the guards around it are uniform).
__device__ __forceinline__ const bf16x8 *mn_stage(const unsigned char *__restrict__ pk, const MemNetLayout &L, int i, int t,
                                                  bf16x8 *wbuf, int wcap)
{
    const int per = L.ks[i] * 64; // 16-byte units per output tile (wcap >= per, see antsrl_launch_memnet)
    const int tpc = wcap / per;   // whole tiles per staged chunk
    const int tt = t % tpc;
    if (tt == 0) {
        const int n = min(tpc, L.tout[i] - t) * per, nt = blockDim.x;
        const bf16x8 *src = reinterpret_cast<const bf16x8 *>(pk + L.frag_off[i]) + (size_t)t * per;
        __syncthreads(); // every wave is done with the previous chunk
        for (int e0 = 0; e0 < n; e0 += MN_SBATCH * nt) {
            bf16x8 v[MN_SBATCH]; // MN_SBATCH loads in flight per thread, then the stores
#pragma unroll
            for (int j = 0; j < MN_SBATCH; ++j) v[j] = src[min(e0 + j * nt + (int)threadIdx.x, n - 1)];
#pragma unroll
            for (int j = 0; j < MN_SBATCH; ++j)
                if (e0 + j * nt + (int)threadIdx.x < n) wbuf[e0 + j * nt + threadIdx.x] = v[j];
        }
        __syncthreads();
    }
    return wbuf + tt * per;
}

// one output tile of a layer whose input is in registers (permuted k order): acc = A . in, A = the tile's staged
// fragments, tin <= MN_MAXT tiles
__device__ __forceinline__ f32x16 mn_tile_reg(const bf16x8 *A, int ks, const bf16x8 (&in)[2 * MN_MAXT], int lane)
{
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    const bf16x8 *a = A + lane;
#pragma unroll
    for (int s = 0; s < 2 * MN_MAXT; ++s) {
        if (s < ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s * 64], in[s], acc, 0, 0, 0);
        if (s % 8 == 7) __builtin_amdgcn_sched_barrier(0); // at most 8 fragments in flight: keeps the wave under 256 VGPRs
    }
    return acc;
}

// one output tile of a layer whose input is the wave's LDS tile (natural k order, ks = Dp / 16 k-steps)
__device__ __forceinline__ f32x16 mn_tile_lds(const bf16x8 *A, int ks, const __bf16 *brow, int lane)
{
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    const bf16x8 *a = A + lane;
    int s = 0;
    for (; s + 4 <= ks; s += 4) {
        bf16x8 av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            av[u] = a[(s + u) * 64];
            bv[u] = *reinterpret_cast<const bf16x8 *>(brow + 16 * (s + u));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[u], bv[u], acc, 0, 0, 0);
    }
    for (; s < ks; ++s) // ks is even (Dp is a multiple of 32): at most one pair left
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s * 64], *reinterpret_cast<const bf16x8 *>(brow + 16 * s), acc, 0, 0, 0);
    return acc;
}

// a whole layer from registers to registers: out = act(A . in + b), rounded to bf16 as the next layer's operand
__device__ __forceinline__ void mn_layer_reg(const unsigned char *__restrict__ pk, const MemNetLayout &L, int i,
                                             const bf16x8 (&in)[2 * MN_MAXT], bf16x8 (&out)[2 * MN_MAXT], bool relu,
                                             int lane, int h, bf16x8 *wbuf, int wcap)
{
    const float *b = reinterpret_cast<const float *>(pk + L.bias_off[i]);
#pragma unroll
    for (int t = 0; t < MN_MAXT; ++t)
        if (t < L.tout[i]) {
            f32x16 acc = mn_tile_reg(mn_stage(pk, L, i, t, wbuf, wcap), L.ks[i], in, lane);
            float bv[16];
            mn_bias(b, t, h, bv);
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[g] = relu ? fmaxf(acc[g] + bv[g], 0.0f) : acc[g] + bv[g];
            mn_to_b(acc, out[2 * t], out[2 * t + 1]);
        }
}

// a whole layer from the LDS tile to registers (L1 with ReLU; R1, P1, M1 without)
__device__ __forceinline__ void mn_layer_lds(const unsigned char *__restrict__ pk, const MemNetLayout &L, int i,
                                             const __bf16 *brow, bf16x8 (&out)[2 * MN_MAXT], bool relu, int lane, int h,
                                             bf16x8 *wbuf, int wcap)
{
    const float *b = reinterpret_cast<const float *>(pk + L.bias_off[i]);
#pragma unroll
    for (int t = 0; t < MN_MAXT; ++t)
        if (t < L.tout[i]) {
            f32x16 acc = mn_tile_lds(mn_stage(pk, L, i, t, wbuf, wcap), L.ks[i], brow, lane);
            float bv[16];
            mn_bias(b, t, h, bv);
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[g] = relu ? fmaxf(acc[g] + bv[g], 0.0f) : acc[g] + bv[g];
            mn_to_b(acc, out[2 * t], out[2 * t + 1]);
        }
}

#ifndef MN_WAVES
#define MN_WAVES 4 // waves per workgroup (32 ants each) sharing every staged weight chunk
#endif
#ifndef MN_WCAP
#define MN_WCAP 4096 // shared weight buffer, 16-byte units (64 KiB; at least one output tile of any layer)
#endif

// host: the forward's launch shape, for antsrl_launch_memnet's kernels and the population's.  wcap = the shared weight
// chunk in 16-byte units (>= one output tile of an x / g layer: Dp / 16 fragments); LDS = one [32][Dp + 8] bf16 tile
// per wave + the chunk, as many waves as fit in 160 KiB, up to MN_WAVES (D <= 320: 4 waves, 146 KiB; D = 1024: 1 wave).
static inline int mn_bf16_wcap(const MemNetLayout &L) { return L.Dp / 16 * 64 > MN_WCAP ? L.Dp / 16 * 64 : MN_WCAP; }
static inline size_t mn_bf16_tile_bytes(const MemNetLayout &L) { return (size_t)32 * (L.Dp + 8) * 2; }
