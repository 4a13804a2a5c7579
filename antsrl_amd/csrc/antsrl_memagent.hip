// antsrl_memagent.hip — the kernels of the memory agent's loop around its net and its training step (include/antsrl.h,
// "The memory agent's loop"; the entries that launch them are in antsrl_memapi.hip): antsrl_agent_select (epsilon-greedy behind antsrl_policy_memory, collect_agent_memory.py:199-204),
// antsrl_agent_plan (the tiles of the batch that hold an ant of a non-exploring environment, for antsrl_policy_memory_tiles) and
// antsrl_replay_record_pre / _post (update_replay_memory + ReplayMemory.extend, :178-187, replay_memory.py:83-114, as two
// gathers of whole rows around the environment step).  The draw specification is written out in include/antsrl.h; the
// device functions of antsrl_draw.h are that text.
//
// k_replay_record: one wave per replay entry.  The entry's ant and ring row are wave-uniform (scalar registers); the
// observation row is copied as 16-byte stores from the first 16-byte boundary of the DESTINATION row on, fed by 16-, 8-
// or 4-byte loads (bfloat16: 8-, 4- or 2-byte) — whatever the source address at that boundary allows, decided per row
// from the two addresses themselves.  (A dense row of 294 floats is 1 176 bytes, so rows alternate between 16- and
// 8-byte alignment; 343 floats are 4-byte aligned only; a "line" pitch makes every source row 128-byte aligned.)  The at
// most 3 + 3 elements in front of and behind the 16-byte body are single stores.  The small per-entry fields (agent
// state ++ memory, the action pair, reward, done) are written by the wave's HIGHEST lanes, which have no vector of the
// row's last, partial round.  No LDS, no scratch, no atomics; ring rows are written with streaming stores (nobody
// re-reads them before a training step samples them).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_memagent_dev.h" // env_explores, load4, load1: what the bodies a population shares (the .inc texts) call

// ------------------------------------------------------------------ antsrl_agent_select
// Part 1: one thread per ant (the actions: antsrl_agent_select_actions.inc).  Part 2: one thread per memory element (V floats),
// coalesced (antsrl_agent_select_memory.inc).  Both are texts a population's select runs too.
template <int V>
__global__ __launch_bounds__(256) void k_agent_select(const SelArgs a)
{
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nthr = (uint64_t)gridDim.x * 256;
#include "antsrl_agent_select_actions.inc"
#include "antsrl_agent_select_memory.inc"
}

// ------------------------------------------------------------------ antsrl_agent_plan
// The list of live 32-ant tiles, ascending.  ONE workgroup of PLAN_THREADS threads walks the T tiles in chunks of
// PLAN_THREADS, one tile per thread: a tile's flag is the OR over its environments (one at n_ants >= 32, as at c3) of
// !env_explores; the flags are ranked by a ballot per wave and a prefix over the chunk's 16 wave counts in LDS (two
// buffers in turn, so one barrier per chunk), and the running base is the same register value in every thread.  One
// workgroup, because the list must be ascending and independent of scheduling without a second launch or a look-back
// chain: c3's 16 384 tiles are 16 chunks of one draw per thread, a few microseconds next to the forward the list
// shortens.  (T grows with M / 32: at 2^31 ants this is 65 536 chunks, still correct, no longer negligible.)
#define PLAN_THREADS 1024

__global__ __launch_bounds__(PLAN_THREADS) void k_agent_plan(const SelArgs a, const uint32_t T, int32_t *__restrict__ tiles,
                                                              int32_t *__restrict__ n_live)
{
    __shared__ uint32_t cnt[2][PLAN_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t c0 = 0, buf = 0; c0 < T; c0 += PLAN_THREADS, buf ^= 1) {
        const uint32_t t = c0 + threadIdx.x;
        bool live = false;
        if (t < T) {
            const uint32_t last = min(32 * t + 31, a.M - 1); // the tile's last ant
            for (uint32_t e = 32 * t / a.n_ants; e <= last / a.n_ants && !live; ++e) live = !env_explores(a, e);
        }
        const uint64_t b = __ballot(live);
        if (lane == 0) cnt[buf][w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t i = 0; i < PLAN_THREADS / 64; ++i) {
            const uint32_t n = cnt[buf][i];
            before += i < w ? n : 0;
            total += n;
        }
        if (live) tiles[base + before + (uint32_t)__popcll(b & ((1ULL << lane) - 1))] = (int32_t)t; // < T: at most t tiles precede t
        base += total;
    }
    if (threadIdx.x == 0) *n_live = (int32_t)base;
}

// ------------------------------------------------------------------ antsrl_replay_record_pre / _post
template <bool BF16, bool POST>
__global__ __launch_bounds__(256) void k_replay_record(const RecArgs a)
{
#include "antsrl_replay_record_body.inc"
}

// ------------------------------------------------------------------ launchers (antsrl_memagent.h)
hipError_t antsrl_launch_agent_select(const SelArgs &a, bool vec, hipStream_t st)
{
    const uint64_t work = a.mem_old == a.mem_next ? a.M : (a.mem_elems > a.M ? a.mem_elems : a.M);
    const unsigned grid = grid_for((size_t)work);
    if (vec)
        hipLaunchKernelGGL(k_agent_select<4>, dim3(grid), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_agent_select<1>, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t antsrl_launch_agent_plan(const SelArgs &a, int32_t *tiles, int32_t *n_live, hipStream_t st)
{
    const uint32_t T = (a.M >> 5) + ((a.M & 31) != 0);
    hipLaunchKernelGGL(k_agent_plan, dim3(1), dim3(PLAN_THREADS), 0, st, a, T, tiles, n_live);
    return hipGetLastError();
}

hipError_t antsrl_launch_replay_record(const RecArgs &a, bool obs_bf16, bool post, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n_write + 3) / 4)), block(256); // <= 2^31 / 4 blocks of 4 waves
    if (!post && obs_bf16)
        hipLaunchKernelGGL((k_replay_record<true, false>), grid, block, 0, st, a);
    else if (!post)
        hipLaunchKernelGGL((k_replay_record<false, false>), grid, block, 0, st, a);
    else if (obs_bf16)
        hipLaunchKernelGGL((k_replay_record<true, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_replay_record<false, true>), grid, block, 0, st, a);
    return hipGetLastError();
}
