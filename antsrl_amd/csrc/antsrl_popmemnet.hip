// antsrl_popmemnet.hip — the acting net of a population of memory agents: P memory nets' bf16 forward in one launch, each
// member with its own pack on its own rows (include/antsrl.h, "The population of memory nets").
//
// k_pop_memnet<OBS16> is k_memnet with the member taken from the grid: grid (ceil(Mm / (32 nw)), P), the member is
// blockIdx.y.  It moves the single forward's arguments (filled by the host for MEMBER 0, io.M = Mm) to its member — the
// pack by the pack stride, obs by Mm F elements of its type, agent_state, mem_in, mem_out, rot, ph and q_out by the
// member's rows — and then runs k_memnet's own text (antsrl_memnet_body.inc) on them.  With io.M = Mm a wave's clamp
// min(t0 + r, M - 1) and its `live` test stay inside the member: a member's last, partial tile reads and writes that
// member's rows only, and its spare waves (t0 >= Mm) run on the member's last ant and write nothing.  A workgroup
// stages one member's weights only; no workgroup straddles members.  So member p's outputs are, bit for bit, what
// antsrl_policy_memory gives on the member's slice with the member's pack.  No atomics; no workgroup reads what
// another writes (mem_in == mem_out is the single forward's in-place rule per ant).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_lds_optin.h"
#include "antsrl_memnet.h"
#include "antsrl_memnet_dev.h"
#include "antsrl_memnet_bf16_dev.h"
#include "antsrl_population.h"

template <bool OBS16>
__global__ void __launch_bounds__(64 * MN_WAVES) // k_memnet's: one workgroup per CU at D <= 320 (LDS)
k_pop_memnet(const unsigned char *__restrict__ pk0, const MemNetIO io0, MemNetDims d, MemNetLayout L, int wcap,
             const size_t pack_stride)
{
    // the body's names, for this member
    const size_t member = blockIdx.y, row0 = member * (size_t)io0.M;
    const unsigned char *__restrict__ pk = pk0 + member * pack_stride;
    MemNetIO io = io0;
    io.obs = reinterpret_cast<const unsigned char *>(io0.obs) + row0 * (size_t)d.F * (OBS16 ? 2 : 4);
    io.agent_state = io0.agent_state + row0 * (size_t)d.A;
    io.mem_in = io0.mem_in + row0 * (size_t)d.mem;
    io.mem_out = io0.mem_out + row0 * (size_t)d.mem;
    io.q_out = io0.q_out ? io0.q_out + row0 * (size_t)(d.n_rot + d.n_ph) : nullptr;
    io.rot = io0.rot + row0;
    io.ph = io0.ph ? io0.ph + row0 : nullptr;

    // k_memnet's prologue without a tile list: wave w of the member's grid row on the member's ants 32 w .. 32 w + 31
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int Dp = L.Dp, stride = Dp + 8; // 16-byte aligned rows, 4-bank skew per row
    __bf16 *xt = reinterpret_cast<__bf16 *>(smem) + (size_t)wib * 32 * stride;        // this wave's [32][Dp + 8]: x, then g
    bf16x8 *wbuf = reinterpret_cast<bf16x8 *>(smem + (size_t)nw * 32 * stride * 2);   // shared weight chunk, wcap units
    const int t0 = (blockIdx.x * nw + wib) * 32;
    const size_t ant = (size_t)min(t0 + r, io.M - 1); // clamped to the MEMBER's last ant: duplicates are not written back
    const bool live = t0 + r < io.M;

#include "antsrl_memnet_body.inc"
}

// antsrl_launch_memnet's rules (LDS, wcap, the waves per workgroup: antsrl_memnet_bf16_dev.h, mn_launch) on a grid
// (ceil(Mm / (32 nw)), P), with the LDS opt-in for this kernel
hipError_t antsrl_launch_pop_memnet(const unsigned char *packs, size_t pack_stride, const MemNetDims &d, const void *obs,
                                    bool obs_bf16, const float *agent_state, const float *mem_in, int Mm, int P,
                                    float *mem_out, int8_t *rot, int8_t *ph, float *q_out, hipStream_t st)
{
    if (Mm < 1 || P < 1 || P > ANTSRL_POP_MAX) return hipErrorInvalidValue;
    MemNetLayout L;
    antsrl_memnet_layout(d, &L);
    const MemNetIO io{obs, agent_state, mem_in, mem_out, q_out, rot, ph, Mm};
    const int wcap = mn_bf16_wcap(L);
    const size_t tile = mn_bf16_tile_bytes(L), shared = (size_t)wcap * 16;
    int nw = MN_WAVES;
    while (nw > 1 && nw * tile + shared > 160 * 1024) --nw;
    const size_t lds = nw * tile + shared;
    const dim3 grid((unsigned)((Mm + 32 * nw - 1) / (32 * nw)), (unsigned)P);
    const hipError_t e = obs_bf16 ? antsrl_lds_optin<k_pop_memnet<true>>(lds) : antsrl_lds_optin<k_pop_memnet<false>>(lds);
    if (e != hipSuccess) return e;
    if (obs_bf16)
        hipLaunchKernelGGL(k_pop_memnet<true>, grid, dim3(64 * nw), lds, st, packs, io, d, L, wcap, pack_stride);
    else
        hipLaunchKernelGGL(k_pop_memnet<false>, grid, dim3(64 * nw), lds, st, packs, io, d, L, wcap, pack_stride);
    return hipGetLastError();
}
