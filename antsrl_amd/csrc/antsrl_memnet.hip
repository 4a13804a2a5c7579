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
// LDS hand-off and the launcher.  Shared with k_pop_memnet (antsrl_popmemnet.hip: the forward of a population's members,
// the member taken from the grid): the helpers of antsrl_memnet_bf16_dev.h and the forward's body, antsrl_memnet_body.inc.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_memnet.h"
#include "antsrl_memnet_dev.h"
#include "antsrl_memnet_bf16_dev.h" // bf16x8, mn_stage, the tile products and layer walks, MN_WAVES, MN_WCAP

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

#include "antsrl_memnet_body.inc"
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
    const int wcap = mn_bf16_wcap(L); // (the LDS rule: antsrl_memnet_bf16_dev.h)
    return mn_launch<k_memnet<true>, k_memnet<false>>(pack, io, d, L, obs_bf16, MN_WAVES, mn_bf16_tile_bytes(L),
                                                      (size_t)wcap * 16, st, wcap);
}

hipError_t antsrl_launch_memnet_tiles(const unsigned char *pack, const MemNetDims &d, const void *obs, bool obs_bf16,
                                      const float *agent_state, const float *mem_in, int M, float *mem_out, int8_t *rot,
                                      int8_t *ph, float *q_out, const int32_t *tiles, const int32_t *n_live, hipStream_t st)
{
    MemNetLayout L;
    antsrl_memnet_layout(d, &L);
    const MemNetIO io{obs, agent_state, mem_in, mem_out, q_out, rot, ph, M};
    const int wcap = mn_bf16_wcap(L);
    return mn_launch<k_memnet<true, const int32_t *, const int32_t *>, k_memnet<false, const int32_t *, const int32_t *>>(
        pack, io, d, L, obs_bf16, MN_WAVES, mn_bf16_tile_bytes(L), (size_t)wcap * 16, st, wcap, tiles, n_live);
}
