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
#include "antsrl_draw.h" // the draw specification (include/antsrl.h)
#include "antsrl_memagent.h"
#include "antsrl_util.h"

// ------------------------------------------------------------------ antsrl_agent_select
__device__ __forceinline__ bool env_explores(const SelArgs &a, uint32_t e)
{
    return draw_u01(agent_draw(a.seed, ANTSRL_DRAW_EXPLORE, (uint64_t)a.env_base + e, a.step, 0)) < a.epsilon;
}

// Part 1: one thread per ant (the actions).  Part 2: one thread per memory element (V floats), coalesced.
template <int V>
__global__ __launch_bounds__(256) void k_agent_select(const SelArgs a)
{
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nthr = (uint64_t)gridDim.x * 256;
    for (uint64_t i = tid; i < a.M; i += nthr) {
        const uint32_t e = (uint32_t)i / a.n_ants, ai = (uint32_t)i - e * a.n_ants;
        const bool ex = env_explores(a, e);
        if (ex) {
            const uint64_t env = (uint64_t)a.env_base + e;
            a.rot[i] = (int8_t)((int)draw_below(agent_draw(a.seed, ANTSRL_DRAW_ROTATION, env, a.step, ai), a.n_rot) - (int)(a.n_rot / 2));
            a.ph[i] = (int8_t)draw_below(agent_draw(a.seed, ANTSRL_DRAW_PHEROMONE, env, a.step, ai), a.n_ph);
        }
        if (ai == 0 && a.explored) a.explored[e] = ex ? 1 : 0;
    }
    if (a.mem_old == a.mem_next) return;
    for (uint64_t f = tid; f < a.mem_elems; f += nthr) {
        const uint32_t e = (uint32_t)(f / a.env_elems);
        if (!env_explores(a, e)) continue; // (the draw is cheap next to the forward pass this follows: kept per element)
        if (V == 4)
            reinterpret_cast<float4 *>(a.mem_next)[f] = reinterpret_cast<const float4 *>(a.mem_old)[f];
        else
            a.mem_next[f] = a.mem_old[f];
    }
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
// 4 consecutive elements at p as floats.  mode 0: one load of the 4 (16 bytes float32, 8 bytes bfloat16), 1: two loads,
// 2: four.  The caller picks the mode from p's alignment.
template <bool BF16>
__device__ __forceinline__ float4 load4(const void *p, int mode)
{
    if (BF16) {
        uint32_t lo, hi;
        if (mode == 0) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p);
            lo = v.x; hi = v.y;
        } else if (mode == 1) {
            lo = reinterpret_cast<const uint32_t *>(p)[0];
            hi = reinterpret_cast<const uint32_t *>(p)[1];
        } else {
            const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
            lo = (uint32_t)q[0] | ((uint32_t)q[1] << 16);
            hi = (uint32_t)q[2] | ((uint32_t)q[3] << 16);
        }
        return make_float4(__uint_as_float(lo << 16), __uint_as_float(lo & 0xFFFF0000u), __uint_as_float(hi << 16),
                           __uint_as_float(hi & 0xFFFF0000u));
    }
    if (mode == 0) return *reinterpret_cast<const float4 *>(p);
    if (mode == 1) {
        const float2 l = reinterpret_cast<const float2 *>(p)[0], h = reinterpret_cast<const float2 *>(p)[1];
        return make_float4(l.x, l.y, h.x, h.y);
    }
    const float *q = reinterpret_cast<const float *>(p);
    return make_float4(q[0], q[1], q[2], q[3]);
}

template <bool BF16>
__device__ __forceinline__ float load1(const void *base, int i)
{
    if (BF16) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(base)[i] << 16);
    return reinterpret_cast<const float *>(base)[i];
}

template <bool BF16, bool POST>
__global__ __launch_bounds__(256) void k_replay_record(const RecArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= a.n_write) return;
    const long long j = a.j0 + w;
    long long row = a.row0 + w;
    if (row >= a.max_len) row -= a.max_len;
    long long ant = j; // K == M: the identity
    if (a.K != a.M) {
        const long long lo = j * a.M / a.K, hi = (j + 1) * a.M / a.K, n = hi - lo;
        long long off = 0;
        if (n > 1) {
            const double u = draw_u01(agent_draw(a.seed, ANTSRL_DRAW_SAMPLE, a.env_base, a.step, (uint64_t)j));
            off = (long long)floor(u * (double)n);
            if (off > n - 1) off = n - 1;
        }
        ant = lo + off;
    }

    // ---- the observation row
    const int F = a.F;
    const size_t esz = BF16 ? 2 : 4;
    const unsigned char *src = reinterpret_cast<const unsigned char *>(a.obs) + (size_t)ant * (size_t)a.pitch * esz;
    float *dst = a.states + (size_t)row * F;
    int h = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2); // elements in front of dst's first 16-byte boundary
    if (h > F) h = F;
    const int nvec = (F - h) >> 2, t0 = h + 4 * nvec;
    if (lane < h)
        dst[lane] = load1<BF16>(src, lane);
    else if (t0 + (lane - h) < F)
        dst[t0 + (lane - h)] = load1<BF16>(src, t0 + (lane - h));
    const unsigned char *sb = src + (size_t)h * esz;
    const uintptr_t sa = (uintptr_t)sb;
    const int mode = BF16 ? ((sa & 7) == 0 ? 0 : (sa & 3) == 0 ? 1 : 2) : ((sa & 15) == 0 ? 0 : (sa & 7) == 0 ? 1 : 2);
    float4 *dv = reinterpret_cast<float4 *>(dst + h);
    for (int v = lane; v < nvec; v += 128) { // two rounds of loads in flight before the stores
        const bool two = v + 64 < nvec;
        const float4 x0 = load4<BF16>(sb + (size_t)v * 4 * esz, mode);
        float4 x1 = x0;
        if (two) x1 = load4<BF16>(sb + (size_t)(v + 64) * 4 * esz, mode);
        store_stream(&dv[v], x0);
        if (two) store_stream(&dv[v + 64], x1);
    }

    // ---- the small fields, on the highest lanes
    const int c = 63 - lane, AM = a.A + a.mem;
    if (c < AM)
        a.agent_states[(size_t)row * AM + c] = c < a.A ? a.agent_state[(size_t)ant * a.A + c] : a.memory[(size_t)ant * a.mem + (c - a.A)];
    if (POST) {
        if (c == 0) a.rewards[row] = a.reward[ant];
        if (c == 1) a.dones[row] = a.done[(uint32_t)ant / (uint32_t)a.n_ants] ? 1 : 0;
    } else {
        if (c == 0) a.actions[2 * row] = (int64_t)a.rot[ant] + a.half_rot;
        if (c == 1) a.actions[2 * row + 1] = a.ph ? (int64_t)a.ph[ant] : 1;
    }
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
