// antsrl_memagent.hip — the memory agent's loop around its net and its training step (include/antsrl.h, "The memory
// agent's loop"): antsrl_agent_select (epsilon-greedy behind antsrl_policy_memory, collect_agent_memory.py:199-204) and
// antsrl_replay_record_pre / _post (update_replay_memory + ReplayMemory.extend, :178-187, replay_memory.py:83-114, as two
// gathers of whole rows around the environment step).  The draw specification is written out in include/antsrl.h; the
// device functions below are that text.
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
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "antsrl_util.h"

__attribute__((visibility("hidden"))) int antsrl_fail_msg(int code, const char *msg); // antsrl_capi.hip: sets antsrl_last_error()

static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return antsrl_fail_msg(code, buf);
}

// ------------------------------------------------------------------ the draw specification (include/antsrl.h)
__device__ __forceinline__ uint64_t agent_draw(uint64_t seed, uint64_t tag, uint64_t env, uint64_t step, uint64_t item)
{
    uint64_t k = mix64(seed + 0x9E3779B97F4A7C15ULL * (env + 1));
    k = mix64(k ^ (0xD1B54A32D192ED03ULL * (step + 1)));
    k = mix64(k + 0x9E3779B97F4A7C15ULL * (item + 1));
    return mix64(k ^ tag);
}
__device__ __forceinline__ double draw_u01(uint64_t k) { return (double)(k >> 11) * (1.0 / 9007199254740992.0); }
__device__ __forceinline__ uint32_t draw_below(uint64_t k, uint32_t n) { return (uint32_t)(((k >> 32) * (uint64_t)n) >> 32); }

// ------------------------------------------------------------------ antsrl_agent_select
struct SelArgs {
    uint64_t seed, step;
    double epsilon;
    int8_t *rot, *ph;
    const float *mem_old;
    float *mem_next;
    uint8_t *explored;
    uint32_t env_base, n_ants, n_rot, n_ph;
    uint32_t M;         // ants
    uint32_t env_elems; // memory elements (floats, or float4 when V == 4) per environment
    uint64_t mem_elems; // memory elements of the batch
};

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

// ------------------------------------------------------------------ antsrl_replay_record_pre / _post
struct RecArgs {
    const void *obs;
    const float *agent_state, *memory, *reward;
    const int8_t *rot, *ph;
    const uint8_t *done;
    float *states, *agent_states, *rewards; // (new_states / new_agent_states in the post half)
    int64_t *actions;
    uint8_t *dones;
    uint64_t seed, step, env_base;
    long long M, K;
    long long j0, n_write; // entries j0 .. j0 + n_write - 1 are written (n_write <= max_len)
    long long row0, max_len; // ring row of entry j0
    long long pitch;       // elements between two ants' observation rows
    int n_ants, F, A, mem, half_rot;
};

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

// ------------------------------------------------------------------ the C ABI
static int check_batch(const char *who, int32_t env_id_base, int32_t n_envs, int32_t n_ants)
{
    if (n_envs < 1 || n_ants < 1) return fail(ANTSRL_E_INVALID, "%s: n_envs and n_ants must be >= 1 (%d, %d)", who, n_envs, n_ants);
    if ((long long)n_envs * n_ants > 0x7fffffffLL)
        return fail(ANTSRL_E_INVALID, "%s: n_envs * n_ants = %lld must stay below 2^31", who, (long long)n_envs * n_ants);
    if (env_id_base < 0 || (long long)env_id_base + n_envs > 0x7fffffffLL)
        return fail(ANTSRL_E_INVALID, "%s: env_id_base must be >= 0 and env_id_base + n_envs must fit 31 bits", who);
    return ANTSRL_OK;
}

static int check_width(const char *who, const char *name, int32_t v)
{
    if (v < 1) return fail(ANTSRL_E_INVALID, "%s: %s must be >= 1 (%d)", who, name, v);
    if (v > 32) return fail(ANTSRL_E_UNSUPPORTED, "%s: %s %d > 32", who, name, v);
    return ANTSRL_OK;
}

#define MISALIGNED(p, n) (((uintptr_t)(p) & ((n) - 1)) != 0)

extern "C" int antsrl_agent_select(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants,
                                   double epsilon, int32_t n_rot, int32_t n_ph, int32_t mem_size, int8_t *rotation,
                                   int8_t *pheromone, const float *mem_old, float *mem_next, uint8_t *explored, void *stream)
{
    const char *who = "agent_select";
    int rc = check_batch(who, env_id_base, n_envs, n_ants);
    if (rc == ANTSRL_OK) rc = check_width(who, "n_rot", n_rot);
    if (rc == ANTSRL_OK) rc = check_width(who, "n_ph", n_ph);
    if (rc == ANTSRL_OK) rc = check_width(who, "mem_size", mem_size);
    if (rc != ANTSRL_OK) return rc;
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(ANTSRL_E_INVALID, "%s: epsilon must be in [0, 1] (%g)", who, epsilon);
    if (!rotation) return fail(ANTSRL_E_INVALID, "%s: rotation is required", who);
    if (!pheromone) return fail(ANTSRL_E_INVALID, "%s: pheromone is required", who);
    if (!mem_old) return fail(ANTSRL_E_INVALID, "%s: mem_old is required", who);
    if (!mem_next) return fail(ANTSRL_E_INVALID, "%s: mem_next is required", who);
    if (MISALIGNED(mem_old, 4) || MISALIGNED(mem_next, 4)) return fail(ANTSRL_E_INVALID, "%s: mem_old and mem_next must be 4-byte aligned", who);
    if (mem_old != mem_next) { // the same buffer, or two that do not touch
        const uintptr_t o = (uintptr_t)mem_old, n = (uintptr_t)mem_next;
        const uintptr_t bytes = (uintptr_t)n_envs * (uintptr_t)n_ants * (uintptr_t)mem_size * 4;
        if (o < n + bytes && n < o + bytes) return fail(ANTSRL_E_INVALID, "%s: mem_old and mem_next overlap without being equal", who);
    }
    SelArgs a;
    a.seed = seed; a.step = step; a.epsilon = epsilon;
    a.rot = rotation; a.ph = pheromone; a.mem_old = mem_old; a.mem_next = mem_next; a.explored = explored;
    a.env_base = (uint32_t)env_id_base; a.n_ants = (uint32_t)n_ants; a.n_rot = (uint32_t)n_rot; a.n_ph = (uint32_t)n_ph;
    a.M = (uint32_t)((long long)n_envs * n_ants);
    const uint64_t env_floats = (uint64_t)n_ants * (uint64_t)mem_size;
    const bool vec = env_floats % 4 == 0 && !MISALIGNED(mem_old, 16) && !MISALIGNED(mem_next, 16);
    const uint64_t env_elems = vec ? env_floats / 4 : env_floats;
    if (env_elems > 0xffffffffULL) return fail(ANTSRL_E_UNSUPPORTED, "%s: n_ants * mem_size = %llu is too large", who, (unsigned long long)env_floats);
    a.env_elems = (uint32_t)env_elems;
    a.mem_elems = env_elems * (uint64_t)n_envs;
    const uint64_t work = mem_old == mem_next ? a.M : (a.mem_elems > a.M ? a.mem_elems : a.M);
    const unsigned grid = grid_for((size_t)work);
    if (vec)
        hipLaunchKernelGGL(k_agent_select<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_agent_select<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ANTSRL_E_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return ANTSRL_OK;
}

static int check_spec(const char *who, const AntsRecordSpec *r)
{
    if (!r) return fail(ANTSRL_E_INVALID, "%s: NULL spec", who);
    int rc = check_batch(who, r->env_id_base, r->n_envs, r->n_ants);
    if (rc != ANTSRL_OK) return rc;
    if (r->n_features < 1) return fail(ANTSRL_E_INVALID, "%s: n_features must be >= 1 (%d)", who, r->n_features);
    if ((rc = check_width(who, "agent_dim", r->agent_dim)) != ANTSRL_OK) return rc;
    if ((rc = check_width(who, "mem_size", r->mem_size)) != ANTSRL_OK) return rc;
    if ((rc = check_width(who, "n_rot", r->n_rot)) != ANTSRL_OK) return rc;
    const long long D = (long long)r->n_features + r->agent_dim + r->mem_size;
    if (D > 1024) return fail(ANTSRL_E_UNSUPPORTED, "%s: D = n_features + agent_dim + mem_size = %lld > 1024", who, D);
    if (r->obs_format != ANTSRL_OBS_F32 && r->obs_format != ANTSRL_OBS_BF16)
        return fail(ANTSRL_E_INVALID, "%s: obs_format must be ANTSRL_OBS_F32 or ANTSRL_OBS_BF16 (%d)", who, r->obs_format);
    if (r->obs_pitch != 0 && (r->obs_pitch < r->n_features || r->obs_pitch >= (1 << 24)))
        return fail(ANTSRL_E_INVALID, "%s: obs_pitch %d: 0 (dense) or at least the row's %d elements (and below 2^24)", who,
                    r->obs_pitch, r->n_features);
    const long long M = (long long)r->n_envs * r->n_ants;
    if (r->K < 1 || r->K > M) return fail(ANTSRL_E_INVALID, "%s: K must be in [1, n_envs * n_ants = %lld] (%lld)", who, M, (long long)r->K);
    if (r->max_len < 1) return fail(ANTSRL_E_INVALID, "%s: max_len must be >= 1 (%lld)", who, (long long)r->max_len);
    if (r->max_len > (1LL << 40)) return fail(ANTSRL_E_INVALID, "%s: max_len must be <= 2^40", who);
    if (r->head < 0 || r->head >= r->max_len)
        return fail(ANTSRL_E_INVALID, "%s: head must be in [0, max_len = %lld) (%lld)", who, (long long)r->max_len, (long long)r->head);
    return ANTSRL_OK;
}

static void fill_rec(const AntsRecordSpec *r, RecArgs *a)
{
    a->seed = r->seed; a->step = r->step; a->env_base = (uint64_t)r->env_id_base;
    a->M = (long long)r->n_envs * r->n_ants; a->K = r->K;
    a->n_write = r->K < r->max_len ? r->K : r->max_len; // only the newest max_len entries can survive
    a->j0 = r->K - a->n_write;
    a->row0 = (r->head + a->j0) % r->max_len;
    a->max_len = r->max_len;
    a->pitch = r->obs_pitch ? r->obs_pitch : r->n_features;
    a->n_ants = r->n_ants; a->F = r->n_features; a->A = r->agent_dim; a->mem = r->mem_size; a->half_rot = r->n_rot / 2;
}

template <bool POST>
static int launch_rec(const char *who, const AntsRecordSpec *r, const RecArgs &a, void *stream)
{
    const unsigned grid = (unsigned)((a.n_write + 3) / 4); // <= 2^31 / 4 blocks of 4 waves
    if (r->obs_format == ANTSRL_OBS_BF16)
        hipLaunchKernelGGL((k_replay_record<true, POST>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_replay_record<false, POST>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ANTSRL_E_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return ANTSRL_OK;
}

#define REQUIRE(p, align)                                                                                    \
    do {                                                                                                     \
        if (!(p)) return fail(ANTSRL_E_INVALID, "%s: %s is required", who, #p);                              \
        if (MISALIGNED(p, align)) return fail(ANTSRL_E_INVALID, "%s: %s must be %d-byte aligned", who, #p, (int)(align)); \
    } while (0)

extern "C" int antsrl_replay_record_pre(const AntsRecordSpec *r, const void *obs, const float *agent_state,
                                        const float *memory, const int8_t *rotation, const int8_t *pheromone, float *states,
                                        float *agent_states, int64_t *actions, void *stream)
{
    const char *who = "replay_record_pre";
    const int rc = check_spec(who, r);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(obs, r->obs_format == ANTSRL_OBS_BF16 ? 2 : 4);
    REQUIRE(agent_state, 4);
    REQUIRE(memory, 4);
    REQUIRE(rotation, 1);
    REQUIRE(states, 4);
    REQUIRE(agent_states, 4);
    REQUIRE(actions, 8);
    RecArgs a = {};
    fill_rec(r, &a);
    a.obs = obs; a.agent_state = agent_state; a.memory = memory; a.rot = rotation; a.ph = pheromone;
    a.states = states; a.agent_states = agent_states; a.actions = actions;
    return launch_rec<false>(who, r, a, stream);
}

extern "C" int antsrl_replay_record_post(const AntsRecordSpec *r, const void *obs, const float *agent_state,
                                         const float *memory, const float *reward, const uint8_t *done, float *rewards,
                                         float *new_states, float *new_agent_states, uint8_t *dones, void *stream)
{
    const char *who = "replay_record_post";
    const int rc = check_spec(who, r);
    if (rc != ANTSRL_OK) return rc;
    REQUIRE(obs, r->obs_format == ANTSRL_OBS_BF16 ? 2 : 4);
    REQUIRE(agent_state, 4);
    REQUIRE(memory, 4);
    REQUIRE(reward, 4);
    REQUIRE(done, 1);
    REQUIRE(rewards, 4);
    REQUIRE(new_states, 4);
    REQUIRE(new_agent_states, 4);
    REQUIRE(dones, 1);
    RecArgs a = {};
    fill_rec(r, &a);
    a.obs = obs; a.agent_state = agent_state; a.memory = memory; a.reward = reward; a.done = done;
    a.rewards = rewards; a.states = new_states; a.agent_states = new_agent_states; a.dones = dones;
    return launch_rec<true>(who, r, a, stream);
}
