// antsrl_memnet_f32.hip — the memory agent net's forward with fp32 MFMA operands (ANTSRL_MEMNET_FP32): the same net,
// shapes and outputs as k_memnet (antsrl_memnet.hip), evaluated with v_mfma_f32_32x32x2_f32, so that nothing is rounded
// to bf16 anywhere.  What the two kernels share is in antsrl_memnet_dev.h.
//
// Precision contract (what tests/memory_policy_ref.py::fp32_forward restates, up to fp32 summation order):
//  - MFMA operands are fp32 (weights, x, the hidden values, g, the head intermediates), accumulation fp32;
//  - biases, ReLU, the residual (L4(...) + b4) + x, tanh, sigmoid and the memory blend are fp32, as in k_memnet;
//  - bf16 observations are widened exactly, then treated as above; the carried memory is never rounded.
// Each 32x32x2 result is a k-ordered fmaf chain.  Every output tile is summed by two such chains (the even and the odd
// k-steps of each group of four), added once at the end: a fixed order, so an ant's result depends on nothing but its
// own inputs (not on M, its place in the batch, or in-place versus out-of-place memory).
//
// Layout.  Each wave owns 32 ants and every layer is computed transposed (W . X^T), as in k_memnet.  For 32x32x2 the B
// operand of lane l is X[k = l >> 5][ant l & 31], and the accumulator register g of lane (r, h) holds row
// (g & 3) + 8 (g >> 2) + 4 h of ant r: register g of tile t is already the B operand of one k-step, with the k pair
// {32 t + 8 (g >> 2) + (g & 3), + 4}.  So hidden widths <= 256 stay in registers with no rounding and no lane movement.
// A k-group q is 4 k-steps (8 inputs): lane (i, h) holds W[row i][8 q + 4 h + u] in element u = 0..3, one 16-byte
// fragment per lane and group (k_memnet_pack_f32; 1 KiB per 32 rows x 8 inputs, 4 bytes per weight).  Register g of
// tile t is element g & 3 of group 4 t + (g >> 2).  The layers fed from x / g (L1, R1, P1, M1) read the same k order
// from the wave's LDS tile: one ds_read_b128 gives a lane x[ant r][8 q + 4 h .. + 3], the B operands of 4 MFMAs.
//
// LDS and weights.  The wave's tile is fp32 [32 ants][Dp], with no padding (Dp = D rounded up to 32): 16-byte chunk
// c of row r sits at chunk c ^ (r & 7), which keeps the b128 reads and writes off each other's banks.  That is 40 KiB
// at Dp = 320, so 4 waves fill the 160 KiB of a CU exactly; D = 1024 runs one wave (128 KiB).  No weight chunk is
// staged in LDS: each wave streams its A fragments from L2 (the packed net is 1.1 MB at power 5, 0.46 MB at power 4)
// with M32_PF groups in flight.  A 32x32x2 step takes 64 cycles against 256 bytes of A per wave, 16 B/clk per CU:
// the MFMA pipe, not the load path, is meant to bound it.  DESIGN §7.8 has the measurements.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_memnet.h"
#include "antsrl_memnet_dev.h"

#define M32_MAXT 8 // hidden tiles held in registers: widths <= 256
#define M32_PF 4   // k-groups of A fragments in flight (one group = 4 MFMAs = 256 cycles)
#ifndef M32_WAVES
#define M32_WAVES 4 // waves per workgroup, as many as the LDS tiles allow
#endif

bool antsrl_memnet_layout_f32(const MemNetDims &d, MemNetLayout *L) { return mn_layout(d, 8, L); } // ks = k-groups of 8 inputs

__global__ void __launch_bounds__(64)
k_memnet_pack_f32(unsigned char *__restrict__ pack, MemNetParams P, MemNetDims d, MemNetLayout L)
{
    const int i = blockIdx.y; // packed layer
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int in_real[MN_NLAYERS] = {d.D, d.h2, d.h3, d.h1, d.D, d.h2, d.h3, d.D, d.h1, d.D, d.h2, d.h2};
    const int nfrag = L.tout[i] * L.ks[i];
    f32x4 *frag = reinterpret_cast<f32x4 *>(pack + L.frag_off[i]);
    for (int f = blockIdx.x; f < nfrag; f += gridDim.x) {
        const int t = f / L.ks[i], q = f % L.ks[i];
        int row;
        const int src = mn_src(i, 32 * t + r, d, &row);
        f32x4 a;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = 8 * q + 4 * h + u;
            a[u] = (src >= 0 && k < in_real[i]) ? P.p[2 * src][(size_t)row * in_real[i] + k] : 0.0f;
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
// column k of row `row` in the wave's LDS tile (16-byte chunks XOR-swizzled by row & 7, within each 32-float block)
__device__ __forceinline__ int m32_swz(int row, int k) { return (((k >> 2) ^ (row & 7)) << 2) | (k & 3); }

__device__ __forceinline__ f32x16 m32_zero()
{
    f32x16 z;
#pragma unroll
    for (int g = 0; g < 16; ++g) z[g] = 0.0f;
    return z;
}

// one output tile of a layer whose input is in registers: A = the tile's fragments (+ lane), ng = 4 x input tiles
__device__ __forceinline__ f32x16 m32_tile_reg(const f32x4 *__restrict__ A, int ng, const f32x16 (&in)[M32_MAXT])
{
    f32x16 e = m32_zero(), o = m32_zero(); // even and odd k-steps of each group
    f32x4 w[M32_PF];
#pragma unroll
    for (int j = 0; j < M32_PF; ++j) w[j] = A[j * 64]; // ng >= 4
#pragma unroll
    for (int t = 0; t < M32_MAXT; ++t)
        if (4 * t < ng) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { // group q = 4 t + j sits in slot j (M32_PF == 4)
                const f32x4 c = w[j];
                w[j] = A[min(4 * t + j + M32_PF, ng - 1) * 64];
                e = __builtin_amdgcn_mfma_f32_32x32x2f32(c[0], in[t][4 * j + 0], e, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(c[1], in[t][4 * j + 1], o, 0, 0, 0);
                e = __builtin_amdgcn_mfma_f32_32x32x2f32(c[2], in[t][4 * j + 2], e, 0, 0, 0);
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(c[3], in[t][4 * j + 3], o, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0); // keeps the loads M32_PF groups ahead, not all hoisted
            }
        }
    return e + o;
}

// one output tile of a layer whose input is the wave's LDS tile (ng = Dp / 8 groups, a multiple of 4); xrow = row r
__device__ __forceinline__ f32x16 m32_tile_lds(const f32x4 *__restrict__ A, int ng, const float *xrow, int r, int h)
{
    f32x16 e = m32_zero(), o = m32_zero();
    f32x4 w[M32_PF];
#pragma unroll
    for (int j = 0; j < M32_PF; ++j) w[j] = A[j * 64];
    f32x4 b = *reinterpret_cast<const f32x4 *>(xrow + ((h ^ (r & 7)) << 2));
    for (int q0 = 0; q0 < ng; q0 += M32_PF) {
#pragma unroll
        for (int j = 0; j < M32_PF; ++j) {
            const int q = q0 + j;
            const f32x4 c = w[j], bc = b;
            w[j] = A[min(q + M32_PF, ng - 1) * 64];
            const int qn = min(q + 1, ng - 1); // the next group's B, one group ahead
            b = *reinterpret_cast<const f32x4 *>(xrow + (((2 * qn + h) ^ (r & 7)) << 2));
            e = __builtin_amdgcn_mfma_f32_32x32x2f32(c[0], bc[0], e, 0, 0, 0);
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(c[1], bc[1], o, 0, 0, 0);
            e = __builtin_amdgcn_mfma_f32_32x32x2f32(c[2], bc[2], e, 0, 0, 0);
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(c[3], bc[3], o, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    return e + o;
}

// acc + bias (+ ReLU) into out[t]: t is uniform, so only one tile's registers are written
__device__ __forceinline__ void m32_put(f32x16 acc, const float *__restrict__ b, int t, int h, bool relu,
                                        f32x16 (&out)[M32_MAXT])
{
    float bv[16];
    mn_bias(b, t, h, bv);
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = relu ? fmaxf(acc[g] + bv[g], 0.0f) : acc[g] + bv[g];
#pragma unroll
    for (int tt = 0; tt < M32_MAXT; ++tt)
        if (tt == t) out[tt] = acc;
}

// a whole layer from registers to registers (output tiles in a loop: one copy of the unrolled k chain per layer)
__device__ __forceinline__ void m32_layer_reg(const unsigned char *__restrict__ pk, const MemNetLayout &L, int i,
                                              const f32x16 (&in)[M32_MAXT], f32x16 (&out)[M32_MAXT], bool relu, int lane,
                                              int h)
{
    const f32x4 *A = reinterpret_cast<const f32x4 *>(pk + L.frag_off[i]) + lane;
    const float *b = reinterpret_cast<const float *>(pk + L.bias_off[i]);
    const int ng = L.ks[i];
    for (int t = 0; t < L.tout[i]; ++t) m32_put(m32_tile_reg(A + (size_t)t * ng * 64, ng, in), b, t, h, relu, out);
}

// a whole layer from the LDS tile to registers (L1 with ReLU; R1, P1, M1 without)
__device__ __forceinline__ void m32_layer_lds(const unsigned char *__restrict__ pk, const MemNetLayout &L, int i,
                                              const float *xrow, f32x16 (&out)[M32_MAXT], bool relu, int lane, int r, int h)
{
    const f32x4 *A = reinterpret_cast<const f32x4 *>(pk + L.frag_off[i]) + lane;
    const float *b = reinterpret_cast<const float *>(pk + L.bias_off[i]);
    const int ng = L.ks[i];
    for (int t = 0; t < L.tout[i]; ++t) m32_put(m32_tile_lds(A + (size_t)t * ng * 64, ng, xrow, r, h), b, t, h, relu, out);
}

// a head's one output tile (R3, P2, M3, Fg): acc + bias
__device__ __forceinline__ f32x16 m32_head(const unsigned char *__restrict__ pk, const MemNetLayout &L, int i, int t,
                                           const f32x16 (&in)[M32_MAXT], int lane, int h)
{
    const int ng = L.ks[i];
    f32x16 q = m32_tile_reg(reinterpret_cast<const f32x4 *>(pk + L.frag_off[i]) + lane + (size_t)t * ng * 64, ng, in);
    float bv[16];
    mn_bias(reinterpret_cast<const float *>(pk + L.bias_off[i]), t, h, bv);
#pragma unroll
    for (int g = 0; g < 16; ++g) q[g] += bv[g];
    return q;
}

// List = nothing: the whole batch; List = (const int32_t *tiles, const int32_t *n_live): the tile-list forward, as in
// k_memnet (antsrl_memnet.hip).
template <bool OBS16, typename... List>
__global__ void __launch_bounds__(64 * M32_WAVES) // one wave per SIMD at D <= 320 (LDS): up to 512 registers
k_memnet_f32(const unsigned char *__restrict__ pk, MemNetIO io, MemNetDims d, MemNetLayout L, List... list)
{
    extern __shared__ __align__(16) float smem32[];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int Dp = L.Dp;
    float *xt = smem32 + (size_t)wib * 32 * Dp; // this wave's [32][Dp] (swizzled): x, then g
    int t0 = (blockIdx.x * nw + wib) * 32;
    bool on = true; // false: a spare wave of a partly filled tile-list workgroup, which writes nothing
    if constexpr (sizeof...(List) != 0)
        if (!mn_list_tile(io.M, &t0, &on, list...)) return;
    const size_t ant = (size_t)min(t0 + r, io.M - 1); // clamped: duplicates are not written back
    const bool live = on && t0 + r < io.M;

    // ---- stage x (fp32) in the wave's LDS tile, as k_memnet does: lanes 0-31 on ant 2p, lanes 32-63 on ant 2p + 1
    for (int c = 0; c < Dp / 32; ++c) {
        const int k = 32 * c + r;
        float xv[16];
        if (32 * c + 32 <= d.F) {
#pragma unroll
            for (int p = 0; p < 16; ++p) xv[p] = mn_obs<OBS16>(io, d, (size_t)min(t0 + 2 * p + h, io.M - 1), k);
        } else {
#pragma unroll
            for (int p = 0; p < 16; ++p) xv[p] = mn_x<OBS16>(io, d, (size_t)min(t0 + 2 * p + h, io.M - 1), k);
        }
#pragma unroll
        for (int p = 0; p < 16; ++p) xt[(2 * p + h) * Dp + m32_swz(2 * p + h, k)] = xv[p];
    }
    mn_tile_sync();
    float *xrow = xt + r * Dp;

    f32x16 u[M32_MAXT], v[M32_MAXT];
    // ---- trunk
    m32_layer_lds(pk, L, 0, xrow, u, true, lane, r, h); // L1
    m32_layer_reg(pk, L, 1, u, v, true, lane, h);       // L2
    m32_layer_reg(pk, L, 2, v, u, true, lane, h);       // L3
    mn_tile_sync(); // every lane's L1 reads of x are done before g overwrites it
    {
        // L4 + residual, one output tile at a time, into the LDS tile as g (fp32)
        const f32x4 *A = reinterpret_cast<const f32x4 *>(pk + L.frag_off[3]) + lane;
        const float *b = reinterpret_cast<const float *>(pk + L.bias_off[3]);
        const int ng = L.ks[3];
        for (int t = 0; t < L.tout[3]; ++t) {
            const f32x16 acc = m32_tile_reg(A + (size_t)t * ng * 64, ng, u);
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
                f32x4 gv;
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] = (acc[4 * q + e] + bv[4 * q + e]) + xr[4 * q + e];
                *reinterpret_cast<f32x4 *>(xrow + m32_swz(r, 32 * t + 8 * q + 4 * h)) = gv;
            }
        }
    }
    mn_tile_sync();

    const int nq = d.n_rot + d.n_ph;
    // ---- rotation head: R3(R2(R1(g)))
    {
        m32_layer_lds(pk, L, 4, xrow, u, false, lane, r, h);
        m32_layer_reg(pk, L, 5, u, v, false, lane, h);
        const f32x16 q = m32_head(pk, L, 6, 0, v, lane, h);
        const int ar = mn_argmax(q, d.n_rot, h);
        if (live) {
            if (h == 0) io.rot[ant] = (int8_t)(ar - d.n_rot / 2);
            if (io.q_out) {
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
        m32_layer_lds(pk, L, 7, xrow, u, false, lane, r, h);
        const f32x16 q = m32_head(pk, L, 8, 0, u, lane, h);
        const int ap = mn_argmax(q, d.n_ph, h);
        if (live) {
            if (h == 0 && io.ph) io.ph[ant] = (int8_t)ap;
            if (io.q_out) {
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
        m32_layer_lds(pk, L, 9, xrow, u, false, lane, r, h);
        m32_layer_reg(pk, L, 10, u, v, false, lane, h);
        const f32x16 m3 = m32_head(pk, L, 11, 0, v, lane, h), fg = m32_head(pk, L, 11, 1, v, lane, h);
        float old[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
            old[g] = io.mem_in[ant * d.mem + min(row, d.mem - 1)]; // every read of this ant's row precedes the write
        }
        if (live)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
                const float s = 1.0f / (1.0f + expf(-fg[g]));
                const float nm = tanhf(m3[g]) * s + old[g] * (1.0f - s);
                if (row < d.mem) io.mem_out[ant * d.mem + row] = nm;
            }
    }
}

hipError_t antsrl_launch_memnet_pack_f32(unsigned char *pack, const MemNetParams &P, const MemNetDims &d, hipStream_t st)
{
    MemNetLayout L;
    antsrl_memnet_layout_f32(d, &L);
    hipLaunchKernelGGL(k_memnet_pack_f32, dim3(64, MN_NLAYERS), dim3(64), 0, st, pack, P, d, L);
    return hipGetLastError();
}

hipError_t antsrl_launch_memnet_f32(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                    const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                    int8_t *ph, float *q_out, hipStream_t st)
{
    MemNetLayout L;
    antsrl_memnet_layout_f32(d, &L);
    const MemNetIO io{obs, agent_state, mem_in, mem_out, q_out, rot, ph, M};
    // LDS: one fp32 [32][Dp] tile per wave and nothing shared (D <= 320: 4 waves; D = 1024: 1)
    return mn_launch<k_memnet_f32<true>, k_memnet_f32<false>>(pack, io, d, L, obs_bf16, M32_WAVES, (size_t)32 * L.Dp * 4, 0, st);
}

hipError_t antsrl_launch_memnet_f32_tiles(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                          const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                          int8_t *ph, float *q_out, const int32_t *tiles, const int32_t *n_live,
                                          hipStream_t st)
{
    MemNetLayout L;
    antsrl_memnet_layout_f32(d, &L);
    const MemNetIO io{obs, agent_state, mem_in, mem_out, q_out, rot, ph, M};
    return mn_launch<k_memnet_f32<true, const int32_t *, const int32_t *>, k_memnet_f32<false, const int32_t *, const int32_t *>>(
        pack, io, d, L, obs_bf16, M32_WAVES, (size_t)32 * L.Dp * 4, 0, st, tiles, n_live);
}
