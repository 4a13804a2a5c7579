// antsrl_memnet_dev.h — what the memory agent net's two forward kernels share: k_memnet (bf16 operands, antsrl_memnet.hip)
// and k_memnet_f32 (fp32 operands, antsrl_memnet_f32.hip).  The packed layout, the source rows of a packed layer, the
// forward's pointers, the fp32 input x, biases, the heads' argmax in the 32x32 accumulator layout, the wave-local LDS
// hand-off, the tile-list lookup (mn_list_tile) and the launcher.  The steps inside the kernels (the pack frame, staging x, L4's residual, the epilogues) stay
// written out in each .hip file: moved into a shared helper, each of them changes the compiler's schedule of both kernels
// (sgpr spills 55 -> 70 in k_memnet<false>, 1.7 % on the power-4 forward), and the kernels are to stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_lds_optin.h"
#include "antsrl_memnet.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// the packed layout (private to the library); k_unit = inputs per `ks` unit: 16 (bf16 k-step) or 8 (fp32 k-group)
static inline size_t mn_align(size_t v) { return (v + 255) & ~(size_t)255; }

static inline bool mn_layout(const MemNetDims &d, int k_unit, MemNetLayout *L)
{
    const int Dp = (d.D + 31) / 32 * 32;
    // in width (padded to 32), out tiles, A order
    const int in_w[MN_NLAYERS] = {Dp, d.h2, d.h3, d.h1, Dp, d.h2, d.h3, Dp, d.h1, Dp, d.h2, d.h2};
    const int out_w[MN_NLAYERS] = {d.h2, d.h3, d.h1, Dp, d.h2, d.h3, 32, d.h1, 32, d.h2, d.h2, 64};
    size_t off = 0;
    L->Dp = Dp;
    for (int i = 0; i < MN_NLAYERS; ++i) {
        L->ks[i] = in_w[i] / k_unit;
        L->tout[i] = out_w[i] / 32;
        L->frag_off[i] = off;
        off = mn_align(off + (size_t)L->tout[i] * L->ks[i] * 64 * 16);
        L->bias_off[i] = off;
        off = mn_align(off + (size_t)L->tout[i] * 32 * 4);
    }
    L->bytes = off;
    return true;
}

// source rows of packed layer i: (tensor index in state_dict order, row) of output row o, or -1 for a zero row
__device__ __forceinline__ int mn_src(int i, int o, const MemNetDims &d, int *row)
{
    // state_dict order: layer1..4 (0..3), rotation_layer1..3 (4..6), pheromone_layer1..2 (7..8),
    // memory_layer1..3 (9..11), forget_layer (12); packed layer 11 = memory_layer3 (tile 0) + forget_layer (tile 1)
    const int nrow[MN_NLAYERS] = {d.h2, d.h3, d.h1, d.D, d.h2, d.h3, d.n_rot, d.h1, d.n_ph, d.h2, d.h2, 0};
    if (i == 11) {
        const int t = o >> 5, rr = o & 31;
        *row = rr;
        return rr < d.mem ? 11 + t : -1;
    }
    *row = o;
    return o < nrow[i] ? i : -1;
}

struct MemNetIO {
    const void *obs;
    const float *agent_state, *mem_in;
    float *mem_out, *q_out;
    int8_t *rot, *ph;
    int M;
};

// input d of ant `ant` as fp32: observation, agent_state, old memory, zero pad (unconditional clamped loads + selects)
template <bool OBS16>
__device__ __forceinline__ float mn_x(const MemNetIO &io, const MemNetDims &d, size_t ant, int k)
{
    const int F = d.F, A = d.A;
    float o;
    if constexpr (OBS16)
        o = (float)__builtin_bit_cast(__bf16, reinterpret_cast<const uint16_t *>(io.obs)[ant * F + min(k, F - 1)]);
    else
        o = reinterpret_cast<const float *>(io.obs)[ant * F + min(k, F - 1)];
    const float a = A > 0 ? io.agent_state[ant * A + min(max(k - F, 0), A - 1)] : 0.0f;
    const float m = io.mem_in[ant * d.mem + min(max(k - F - A, 0), d.mem - 1)];
    return k < F ? o : (k < F + A ? a : (k < d.D ? m : 0.0f));
}

// one observation element as fp32 (the chunk is known to lie inside the observation row)
template <bool OBS16>
__device__ __forceinline__ float mn_obs(const MemNetIO &io, const MemNetDims &d, size_t ant, int k)
{
    if constexpr (OBS16)
        return (float)__builtin_bit_cast(__bf16, reinterpret_cast<const uint16_t *>(io.obs)[ant * d.F + k]);
    else
        return reinterpret_cast<const float *>(io.obs)[ant * d.F + k];
}

// bias of the 16 rows lane (., h) holds in output tile t
__device__ __forceinline__ void mn_bias(const float *__restrict__ b, int t, int h, float (&bv)[16])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(b + 32 * t + 8 * q + 4 * h);
        bv[4 * q] = v.x; bv[4 * q + 1] = v.y; bv[4 * q + 2] = v.z; bv[4 * q + 3] = v.w;
    }
}

// first maximum of n <= 32 head outputs of ant r, held as rows (g & 3) + 8 (g >> 2) + 4 h by lanes r and r + 32
__device__ __forceinline__ int mn_argmax(const f32x16 &v, int n, int h)
{
    float best = 0.0f;
    int bi = 1 << 30;
#pragma unroll
    for (int g = 0; g < 16; ++g) { // rows ascend with g: a strict > keeps the first maximum
        const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
        if (row < n && (bi == (1 << 30) || v[g] > best)) { best = v[g]; bi = row; }
    }
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(bi, 32);
    if (oi != (1 << 30) && (bi == (1 << 30) || ob > best || (ob == best && oi < bi))) bi = oi;
    return bi;
}

// wave-local LDS hand-off: every lane's accesses to the wave's tile before it are done before any after it
__device__ __forceinline__ void mn_tile_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The tile-list kernels' place in the batch.  The grid covers all T = ceil(M / 32) tiles, because the host does not know
// *n_live; wave `slot` = blockIdx.x * waves + wave-in-block takes tile tiles[slot].  false: the workgroup's first slot is
// at or beyond n_live (clamped to [0, T]) — uniform over the workgroup, so all of it leaves before any barrier.  Else
// *on says whether this wave has a tile: its slot is below n_live and the entry lies in [0, T).  The entry is compared in
// a scalar register (wave-uniform) before it is ever multiplied into an address; a wave without a tile runs on tile 0's
// inputs (valid addresses, M >= 1) and writes nothing.
__device__ __forceinline__ bool mn_list_tile(int M, int *t0, bool *on, const int32_t *__restrict__ tiles,
                                             const int32_t *__restrict__ n_live)
{
    const int wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int T = (M >> 5) + ((M & 31) != 0);
    const int n = min(max(*n_live, 0), T);
    const int first = blockIdx.x * nw; // < T: the grid has ceil(T / nw) workgroups
    if (first >= n) return false;
    const int slot = first + wib;      // < n <= T inside the branch: within the list's capacity
    const int t = __builtin_amdgcn_readfirstlane(slot < n ? tiles[slot] : -1);
    *on = t >= 0 && t < T;
    *t0 = *on ? t * 32 : 0;
    return true;
}

// host: the launcher.  K16 / K32 = the forward kernel for bfloat16 / float32 observations; LDS = one `tile` per wave
// (32 ants) + `shared` bytes per workgroup, as many waves as fit in 160 KiB, up to max_waves; extra = what the kernel
// takes behind (pack, io, d, L).
template <auto K16, auto K32, typename... Extra>
static hipError_t mn_launch(const unsigned char *pack, const MemNetIO &io, const MemNetDims &d, const MemNetLayout &L,
                            bool obs_bf16, int max_waves, size_t tile, size_t shared, hipStream_t st, Extra... extra)
{
    int nw = max_waves;
    while (nw > 1 && nw * tile + shared > 160 * 1024) --nw;
    const size_t lds = nw * tile + shared;
    const int blocks = (io.M + 32 * nw - 1) / (32 * nw);
    const hipError_t e = obs_bf16 ? antsrl_lds_optin<K16>(lds) : antsrl_lds_optin<K32>(lds);
    if (e != hipSuccess) return e;
    if (obs_bf16)
        hipLaunchKernelGGL(K16, dim3(blocks), dim3(64 * nw), lds, st, pack, io, d, L, extra...);
    else
        hipLaunchKernelGGL(K32, dim3(blocks), dim3(64 * nw), lds, st, pack, io, d, L, extra...);
    return hipGetLastError();
}
