// antsrl_memnet.hip — inference of the reference's recurrent memory agent net, `CollectModelMemory`
// (agents/collect_agent_memory.py:24-78), evaluated on the observation tensor without leaving the device.
//
// Per ant, x = cat[obs.view(F), agent_state(A), old_memory(mem)], D = F + A + mem, widths h1 < h2 < h3:
//     g     = L4(relu(L3(relu(L2(relu(L1(x))))))) + x        (the residual is added BEFORE the three heads)
//     q_rot = R3(R2(R1(g)))      q_ph = P2(P1(g))      m = M2(M1(g))           (no activations in the heads)
//     new_memory = tanh(M3(m)) * s + old_memory * (1 - s),   s = sigmoid(Fg(m))
//     rotation = argmax(q_rot) - n_rot // 2,   pheromone = argmax(q_ph)          (collect_agent_memory.py:195-200)
//
// Precision contract (what tests/memory_policy_ref.py::bf16_forward restates):
//  - MFMA operands are bf16, accumulation fp32 (v_mfma_f32_32x32x16_bf16); the weights are rounded to bf16 once,
//    by k_memnet_pack;
//  - every layer's input is rounded to bf16 at the MFMA (x, the hidden values, g, the head intermediates);
//  - biases, ReLU, the residual add (L4(...) + b4) + x, tanh, sigmoid and the memory blend are fp32;
//  - the residual uses the fp32 x (for bf16 observations: their exact widening);
//  - old_memory is read as fp32 and new_memory written as fp32: the carried memory is never rounded to bf16, only
//    its copy as an operand of L1.
//
// Layout.  A workgroup of up to MN_WAVES waves; each wave owns 32 ants.  Every layer is computed TRANSPOSED,
// W (out x in) . X^T (in x 32 ants), so a lane (r, h) ends up holding 16 outputs of ITS ant r — rows
// (g & 3) + 8 (g >> 2) + 4 h of each 32-row tile — and that accumulator, rounded to bf16, is the next layer's B operand
// without any lane movement (as in k_policy_mlp's heads): register 8 q + j of tile t is input
// k = 32 t + 16 q + 8 (j >> 2) + 4 h + (j & 3) of k-step 2 t + q.  k_memnet_pack stores the A fragments of such layers
// in that permuted k order.  The hidden widths (<= 256) live in registers this way.  x and g (D <= 1024 wide) do not
// fit there: they live in a wave-private LDS tile [32 ants][Dp + 8] of bf16 (Dp = D rounded up to 32), from which the
// B fragments of L1 and of the three heads' first layers are read in natural k order.  x is staged there once
// (coalesced 32-column chunks, the observation-only chunks with one load per element); L4's output tiles g overwrite
// it (L1 has consumed x by then).  The fp32 x of the residual is re-read from global memory (L2-resident: the staging
// pass has just read it).
//
// Weight traffic.  The waves of a workgroup walk the same sequence of layers and output tiles, so the A fragments are
// staged ONCE per workgroup into a shared LDS chunk (MN_WCAP: 64 KiB, as many whole output tiles of a layer as fit)
// and every wave's MFMAs read them from there (mn_stage).  Per MN_WAVES x 32 = 128 ants the packed net (567 808 bytes
// at power 5, 236 032 at power 4, F = 294) is read from L2 once: 2.3 GB per c3 batch at power 5 instead of the 9.3 GB
// of one read per 32 ants.  LDS at D <= 320: 4 x 20.5 KiB of x / g tiles + the 64 KiB chunk = 146 KiB, one workgroup
// per CU.  DESIGN §7.6 has the measurements.
//
// Shared with k_memnet_f32 (antsrl_memnet_dev.h): the packed layout, the input and bias helpers, argmax, the wave-local
// LDS hand-off and the launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_memnet.h"
#include "antsrl_memnet_dev.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

#define MN_MAXT 8 // hidden tiles held in registers: widths <= 256

bool antsrl_memnet_layout(const MemNetDims &d, MemNetLayout *L) { return mn_layout(d, 16, L); } // ks = k-steps of 16 inputs

__global__ void __launch_bounds__(64)
k_memnet_pack(unsigned char *__restrict__ pack, MemNetParams P, MemNetDims d, MemNetLayout L)
{
    const int i = blockIdx.y; // packed layer
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const bool natural = (i == 0 || i == 4 || i == 7 || i == 9); // B from the LDS tile (x / g): natural k order
    const int in_real[MN_NLAYERS] = {d.D, d.h2, d.h3, d.h1, d.D, d.h2, d.h3, d.D, d.h1, d.D, d.h2, d.h2};
    const int nfrag = L.tout[i] * L.ks[i];
    bf16x8 *frag = reinterpret_cast<bf16x8 *>(pack + L.frag_off[i]);
    for (int f = blockIdx.x; f < nfrag; f += gridDim.x) {
        const int t = f / L.ks[i], s = f % L.ks[i];
        int row;
        const int src = mn_src(i, 32 * t + r, d, &row);
        bf16x8 a;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = natural ? 16 * s + 8 * h + j : 16 * s + 8 * (j >> 2) + 4 * h + (j & 3);
            const float w = (src >= 0 && k < in_real[i]) ? P.p[2 * src][(size_t)row * in_real[i] + k] : 0.0f;
            a[j] = (__bf16)w;
        }
        frag[(size_t)f * 64 + lane] = a;
    }
    if (blockIdx.x == 0) {
        float *bias = reinterpret_cast<float *>(pack + L.bias_off[i]);
        for (int o = lane; o < 32 * L.tout[i]; o += 64) {
            int row;
            const int src = mn_src(i, o, d, &row);
            bias[o] = src >= 0 ? P.p[2 * src + 1][row] : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------
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

// List = nothing: the forward over the whole batch, wave w of the grid on ants 32 w .. 32 w + 31 (antsrl_policy_memory).
// List = (const int32_t *tiles, const int32_t *n_live): the tile-list forward (antsrl_policy_memory_tiles), wave w on tile
// tiles[w] (mn_list_tile).  Everything behind t0 is the same code, so a listed tile's results are the full forward's bits.
template <bool OBS16, typename... List>
__global__ void __launch_bounds__(64 * MN_WAVES) // one workgroup per CU at D <= 320 (LDS): one wave per SIMD, 512 registers
k_memnet(const unsigned char *__restrict__ pk, MemNetIO io, MemNetDims d, MemNetLayout L, int wcap, List... list)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int Dp = L.Dp, stride = Dp + 8; // 16-byte aligned rows, 4-bank skew per row
    __bf16 *xt = reinterpret_cast<__bf16 *>(smem) + (size_t)wib * 32 * stride;        // this wave's [32][Dp + 8]: x, then g
    bf16x8 *wbuf = reinterpret_cast<bf16x8 *>(smem + (size_t)nw * 32 * stride * 2);   // shared weight chunk, wcap units
    int t0 = (blockIdx.x * nw + wib) * 32;
    bool on = true; // false: a spare wave of a partly filled tile-list workgroup walks the barriers and writes nothing
    if constexpr (sizeof...(List) != 0)
        if (!mn_list_tile(io.M, &t0, &on, list...)) return; // the whole workgroup, before any barrier
    const size_t ant = (size_t)min(t0 + r, io.M - 1); // clamped: duplicates are not written back
    const bool live = on && t0 + r < io.M;

    // ---- stage x (bf16) in the wave's LDS tile: 32-column chunks, lanes 0-31 on ant 2p and lanes 32-63 on ant 2p + 1
    // (128 coalesced bytes of a float32 row per half-wave), the 16 ant pairs' loads in flight together
    for (int c = 0; c < Dp / 32; ++c) {
        const int k = 32 * c + r;
        float xv[16];
        if (32 * c + 32 <= d.F) { // observation columns only
#pragma unroll
            for (int p = 0; p < 16; ++p) xv[p] = mn_obs<OBS16>(io, d, (size_t)min(t0 + 2 * p + h, io.M - 1), k);
        } else {                  // end of the row, agent_state, old memory, zero pad
#pragma unroll
            for (int p = 0; p < 16; ++p) xv[p] = mn_x<OBS16>(io, d, (size_t)min(t0 + 2 * p + h, io.M - 1), k);
        }
#pragma unroll
        for (int p = 0; p < 16; ++p) xt[(2 * p + h) * stride + k] = (__bf16)xv[p];
    }
    mn_tile_sync();
    const __bf16 *brow = xt + r * stride + 8 * h;

    bf16x8 u[2 * MN_MAXT], v[2 * MN_MAXT];
    // ---- trunk
    mn_layer_lds(pk, L, 0, brow, u, true, lane, h, wbuf, wcap); // L1
    mn_layer_reg(pk, L, 1, u, v, true, lane, h, wbuf, wcap);    // L2
    mn_layer_reg(pk, L, 2, v, u, true, lane, h, wbuf, wcap);    // L3
    mn_tile_sync(); // every lane's L1 reads of x are done before g overwrites it
    {
        // L4 + residual, one output tile at a time, into the LDS tile as g (bf16)
        const float *b = reinterpret_cast<const float *>(pk + L.bias_off[3]);
        for (int t = 0; t < L.tout[3]; ++t) {
            f32x16 acc = mn_tile_reg(mn_stage(pk, L, 3, t, wbuf, wcap), L.ks[3], u, lane);
            float bv[16], xr[16];
            mn_bias(b, t, h, bv);
            if (32 * t + 32 <= d.F) {
#pragma unroll
                for (int g = 0; g < 16; ++g) xr[g] = mn_obs<OBS16>(io, d, ant, 32 * t + (g & 3) + 8 * (g >> 2) + 4 * h);
            } else {
#pragma unroll
                for (int g = 0; g < 16; ++g) xr[g] = mn_x<OBS16>(io, d, ant, 32 * t + (g & 3) + 8 * (g >> 2) + 4 * h);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
                bf16x4 gv;
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] = (__bf16)((acc[4 * q + e] + bv[4 * q + e]) + xr[4 * q + e]);
                *reinterpret_cast<bf16x4 *>(xt + r * stride + 32 * t + 8 * q + 4 * h) = gv;
            }
        }
    }
    mn_tile_sync();

    // ---- rotation head: R3(R2(R1(g)))
    {
        mn_layer_lds(pk, L, 4, brow, u, false, lane, h, wbuf, wcap);
        mn_layer_reg(pk, L, 5, u, v, false, lane, h, wbuf, wcap);
        f32x16 q = mn_tile_reg(mn_stage(pk, L, 6, 0, wbuf, wcap), L.ks[6], v, lane);
        float bv[16];
        mn_bias(reinterpret_cast<const float *>(pk + L.bias_off[6]), 0, h, bv);
#pragma unroll
        for (int g = 0; g < 16; ++g) q[g] += bv[g];
        const int ar = mn_argmax(q, d.n_rot, h);
        if (live) {
            if (h == 0) io.rot[ant] = (int8_t)(ar - d.n_rot / 2);
            if (io.q_out) {
                const int nq = d.n_rot + d.n_ph;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                    if (row < d.n_rot) io.q_out[ant * nq + row] = q[g];
                }
            }
        }
    }
    // ---- pheromone head: P2(P1(g))
    {
        mn_layer_lds(pk, L, 7, brow, u, false, lane, h, wbuf, wcap);
        f32x16 q = mn_tile_reg(mn_stage(pk, L, 8, 0, wbuf, wcap), L.ks[8], u, lane);
        float bv[16];
        mn_bias(reinterpret_cast<const float *>(pk + L.bias_off[8]), 0, h, bv);
#pragma unroll
        for (int g = 0; g < 16; ++g) q[g] += bv[g];
        const int ap = mn_argmax(q, d.n_ph, h);
        if (live) {
            if (h == 0 && io.ph) io.ph[ant] = (int8_t)ap;
            if (io.q_out) {
                const int nq = d.n_rot + d.n_ph;
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                    if (row < d.n_ph) io.q_out[ant * nq + d.n_rot + row] = q[g];
                }
            }
        }
    }
    // ---- memory: m = M2(M1(g)); new = tanh(M3 m) * s + old * (1 - s), s = sigmoid(Fg m)
    {
        mn_layer_lds(pk, L, 9, brow, u, false, lane, h, wbuf, wcap);
        mn_layer_reg(pk, L, 10, u, v, false, lane, h, wbuf, wcap);
        const float *b = reinterpret_cast<const float *>(pk + L.bias_off[11]);
        // both tiles in one staged chunk (2 x ks[11] <= 32 fragments): tile 1 follows tile 0
        const bf16x8 *A = mn_stage(pk, L, 11, 0, wbuf, wcap);
        f32x16 m3 = mn_tile_reg(A, L.ks[11], v, lane), fg = mn_tile_reg(A + L.ks[11] * 64, L.ks[11], v, lane);
        float b3[16], bf[16], old[16];
        mn_bias(b, 0, h, b3);
        mn_bias(b, 1, h, bf);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            old[g] = io.mem_in[ant * d.mem + min(row, d.mem - 1)]; // every read of this ant's row precedes the write
        }
        if (live)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                const float s = 1.0f / (1.0f + expf(-(fg[g] + bf[g])));
                const float nm = tanhf(m3[g] + b3[g]) * s + old[g] * (1.0f - s);
                if (row < d.mem) io.mem_out[ant * d.mem + row] = nm;
            }
    }
}

hipError_t antsrl_launch_memnet_pack(unsigned char *pack, const MemNetParams &P, const MemNetDims &d, hipStream_t st)
{
    MemNetLayout L;
    antsrl_memnet_layout(d, &L);
    hipLaunchKernelGGL(k_memnet_pack, dim3(64, MN_NLAYERS), dim3(64), 0, st, pack, P, d, L);
    return hipGetLastError();
}

hipError_t antsrl_launch_memnet(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                int8_t *ph, float *q_out, hipStream_t st)
{
    MemNetLayout L;
    antsrl_memnet_layout(d, &L);
    const MemNetIO io{obs, agent_state, mem_in, mem_out, q_out, rot, ph, M};
    // LDS: one [32][Dp + 8] bf16 tile per wave + the shared weight chunk (>= one output tile of an x / g layer: Dp / 16
    // fragments): D <= 320: 4 waves, 146 KiB; D = 1024: 1 wave
    const int wcap = L.Dp / 16 * 64 > MN_WCAP ? L.Dp / 16 * 64 : MN_WCAP;
    return mn_launch<k_memnet<true>, k_memnet<false>>(pack, io, d, L, obs_bf16, MN_WAVES, (size_t)32 * (L.Dp + 8) * 2,
                                                      (size_t)wcap * 16, st, wcap);
}

hipError_t antsrl_launch_memnet_tiles(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                      const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                      int8_t *ph, float *q_out, const int32_t *tiles, const int32_t *n_live, hipStream_t st)
{
    MemNetLayout L;
    antsrl_memnet_layout(d, &L);
    const MemNetIO io{obs, agent_state, mem_in, mem_out, q_out, rot, ph, M};
    const int wcap = L.Dp / 16 * 64 > MN_WCAP ? L.Dp / 16 * 64 : MN_WCAP; // as antsrl_launch_memnet
    return mn_launch<k_memnet<true, const int32_t *, const int32_t *>, k_memnet<false, const int32_t *, const int32_t *>>(
        pack, io, d, L, obs_bf16, MN_WAVES, (size_t)32 * (L.Dp + 8) * 2, (size_t)wcap * 16, st, wcap, tiles, n_live);
}
