// antsrl_memapi.hip — the memory agent's net in the C-ABI of libantsrl_hip.so (include/antsrl.h): its inference
// (antsrl_memnet_*, antsrl_policy_memory*) and its training step (antsrl_memtrain_*).  The loop around them is
// antsrl_loopapi.hip's.
//
// Host-side only: validates the arguments and enqueues the kernels of antsrl_memnet.hip / _memnet_f32.hip and
// antsrl_memtrain.hip on the caller's stream.  No handle, no allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_adam.h"
#include "antsrl_device.h"
#include "antsrl_fail.h"
#include "antsrl_loopapi.h" // the shape limits, the obs_format rule
#include "antsrl_memnet.h"
#include "antsrl_memtrain.h"

// the 26 tensors of CollectModelMemory.state_dict(): none NULL
static int check_params(const char *who, const float *const *params)
{
    for (int i = 0; i < 26; ++i)
        if (!params[i]) return fail(ANTSRL_E_INVALID, "%s: params[%d] is NULL", who, i);
    return ANTSRL_OK;
}

// ---- the net (antsrl_memnet.hip, antsrl_memnet_f32.hip)
static int memnet_check(const AntsMemNetShape *s, MemNetDims *d, const char *who)
{
    if (!s) return fail(ANTSRL_E_INVALID, "%s: NULL shape", who);
    if (s->n_features < 1 || s->agent_dim < 1 || s->mem_size < 1 || s->h1 < 1 || s->h2 < 1 || s->h3 < 1 || s->n_rot < 1 ||
        s->n_ph < 1)
        return fail(ANTSRL_E_INVALID, "%s: n_features, agent_dim, mem_size, h1, h2, h3, n_rot, n_ph must be >= 1", who);
    int rc = antsrl_check_D(who, s->n_features, s->agent_dim, s->mem_size);
    if (rc == ANTSRL_OK) rc = antsrl_check_max32(who, "agent_dim", s->agent_dim);
    if (rc == ANTSRL_OK) rc = antsrl_check_max32(who, "mem_size", s->mem_size);
    if (rc != ANTSRL_OK) return rc;
    if (s->h1 % 32 || s->h2 % 32 || s->h3 % 32 || s->h1 > 256 || s->h2 > 256 || s->h3 > 256)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: h1, h2, h3 (%d, %d, %d) must be multiples of 32 and <= 256", who, s->h1, s->h2,
                    s->h3);
    // (n_rot, n_ph <= 32 has its own, combined text here and antsrl_check_max32's in the loop's entries: both are tested)
    if (s->n_rot > 32 || s->n_ph > 32) return fail(ANTSRL_E_UNSUPPORTED, "%s: n_rot, n_ph (%d, %d) must be <= 32", who, s->n_rot, s->n_ph);
    const int D = s->n_features + s->agent_dim + s->mem_size; // <= 1024 (antsrl_check_D)
    *d = MemNetDims{s->n_features, s->agent_dim, s->mem_size, D, s->h1, s->h2, s->h3, s->n_rot, s->n_ph};
    return ANTSRL_OK;
}

// precision: ANTSRL_MEMNET_BF16 (k_memnet) or ANTSRL_MEMNET_FP32 (k_memnet_f32), checked before anything else
static int memnet_precision(int precision, const char *who)
{
    if (precision != ANTSRL_MEMNET_BF16 && precision != ANTSRL_MEMNET_FP32)
        return fail(ANTSRL_E_INVALID, "%s: precision %d is neither ANTSRL_MEMNET_BF16 (0) nor ANTSRL_MEMNET_FP32 (1)", who,
                    precision);
    return ANTSRL_OK;
}

static int memnet_packed_bytes(const AntsMemNetShape *s, int precision, size_t *bytes, const char *who)
{
    MemNetDims d;
    const int rc = memnet_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!bytes) return fail(ANTSRL_E_INVALID, "%s: NULL bytes", who);
    MemNetLayout L;
    if (precision == ANTSRL_MEMNET_FP32)
        antsrl_memnet_layout_f32(d, &L);
    else
        antsrl_memnet_layout(d, &L);
    *bytes = L.bytes;
    return ANTSRL_OK;
}

static int memnet_pack(const AntsMemNetShape *s, int precision, const float *const *params, void *packed, void *stream,
                       const char *who)
{
    MemNetDims d;
    const int rc = memnet_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!params || !packed) return fail(ANTSRL_E_INVALID, "%s: params and packed are required", who);
    if ((uintptr_t)packed & 255) return fail(ANTSRL_E_INVALID, "%s: packed must be 256-byte aligned", who);
    const int prc = check_params(who, params);
    if (prc != ANTSRL_OK) return prc;
    MemNetParams P;
    for (int i = 0; i < 26; ++i) P.p[i] = params[i];
    hipError_t e = precision == ANTSRL_MEMNET_FP32 ? antsrl_launch_memnet_pack_f32((unsigned char *)packed, P, d, (hipStream_t)stream)
                                                   : antsrl_launch_memnet_pack((unsigned char *)packed, P, d, (hipStream_t)stream);
    return enqueued(e, who);
}

static int policy_memory(const AntsMemNetShape *s, int precision, const void *packed, const void *obs, int obs_format,
                         const float *agent_state, const float *mem_in, int64_t n_ants, float *mem_out, int8_t *rotation,
                         int8_t *pheromone, float *q_out, void *stream, const char *who, bool listed = false,
                         const int32_t *tiles = nullptr, const int32_t *n_live = nullptr)
{
    MemNetDims d;
    int rc = memnet_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!packed || !obs || !agent_state || !mem_in || !mem_out || !rotation)
        return fail(ANTSRL_E_INVALID, "%s: packed, obs, agent_state, mem_in, mem_out, rotation are required", who);
    if (listed && (!tiles || !n_live)) return fail(ANTSRL_E_INVALID, "%s: tiles and n_live are required", who);
    if (listed && (((uintptr_t)tiles | (uintptr_t)n_live) & 3))
        return fail(ANTSRL_E_INVALID, "%s: tiles and n_live must be 4-byte aligned", who);
    if ((uintptr_t)packed & 255) return fail(ANTSRL_E_INVALID, "%s: packed must be 256-byte aligned", who);
    if ((rc = antsrl_check_obs_format(who, obs_format)) != ANTSRL_OK) return rc;
    if (n_ants < 1 || n_ants > 0x7fffffff) return fail(ANTSRL_E_INVALID, "%s: n_ants must be in [1, 2^31)", who);
    if (listed)
        return enqueued((precision == ANTSRL_MEMNET_FP32 ? antsrl_launch_memnet_f32_tiles : antsrl_launch_memnet_tiles)(
                            (const unsigned char *)packed, d, obs, obs_format == ANTSRL_OBS_BF16, agent_state, mem_in,
                            (int)n_ants, mem_out, rotation, pheromone, q_out, tiles, n_live, (hipStream_t)stream),
                        who);
    hipError_t e = (precision == ANTSRL_MEMNET_FP32 ? antsrl_launch_memnet_f32 : antsrl_launch_memnet)(
        (const unsigned char *)packed, d, obs, obs_format == ANTSRL_OBS_BF16, agent_state, mem_in, (int)n_ants, mem_out,
        rotation, pheromone, q_out, (hipStream_t)stream);
    return enqueued(e, who);
}

extern "C" int antsrl_memnet_packed_bytes(const AntsMemNetShape *s, size_t *bytes)
{
    return memnet_packed_bytes(s, ANTSRL_MEMNET_BF16, bytes, "memnet_packed_bytes");
}

extern "C" int antsrl_memnet_pack(const AntsMemNetShape *s, const float *const *params, void *packed, void *stream)
{
    return memnet_pack(s, ANTSRL_MEMNET_BF16, params, packed, stream, "memnet_pack");
}

extern "C" int antsrl_policy_memory(const AntsMemNetShape *s, const void *packed, const void *obs, int obs_format,
                                    const float *agent_state, const float *mem_in, int64_t n_ants, float *mem_out,
                                    int8_t *rotation, int8_t *pheromone, float *q_out, void *stream)
{
    return policy_memory(s, ANTSRL_MEMNET_BF16, packed, obs, obs_format, agent_state, mem_in, n_ants, mem_out, rotation,
                         pheromone, q_out, stream, "policy_memory");
}

extern "C" int antsrl_memnet_packed_bytes_ex(const AntsMemNetShape *s, int precision, size_t *bytes)
{
    const int rc = memnet_precision(precision, "memnet_packed_bytes_ex");
    return rc != ANTSRL_OK ? rc : memnet_packed_bytes(s, precision, bytes, "memnet_packed_bytes_ex");
}

extern "C" int antsrl_memnet_pack_ex(const AntsMemNetShape *s, int precision, const float *const *params, void *packed,
                                     void *stream)
{
    const int rc = memnet_precision(precision, "memnet_pack_ex");
    return rc != ANTSRL_OK ? rc : memnet_pack(s, precision, params, packed, stream, "memnet_pack_ex");
}

extern "C" int antsrl_policy_memory_ex(const AntsMemNetShape *s, int precision, const void *packed, const void *obs,
                                       int obs_format, const float *agent_state, const float *mem_in, int64_t n_ants,
                                       float *mem_out, int8_t *rotation, int8_t *pheromone, float *q_out, void *stream)
{
    const int rc = memnet_precision(precision, "policy_memory_ex");
    return rc != ANTSRL_OK ? rc
                           : policy_memory(s, precision, packed, obs, obs_format, agent_state, mem_in, n_ants, mem_out,
                                           rotation, pheromone, q_out, stream, "policy_memory_ex");
}

extern "C" int antsrl_policy_memory_tiles(const AntsMemNetShape *s, int precision, const void *packed, const void *obs,
                                          int obs_format, const float *agent_state, const float *mem_in, int64_t n_ants,
                                          float *mem_out, int8_t *rotation, int8_t *pheromone, float *q_out,
                                          const int32_t *tiles, const int32_t *n_live, void *stream)
{
    const int rc = memnet_precision(precision, "policy_memory_tiles");
    return rc != ANTSRL_OK ? rc
                           : policy_memory(s, precision, packed, obs, obs_format, agent_state, mem_in, n_ants, mem_out,
                                           rotation, pheromone, q_out, stream, "policy_memory_tiles", true, tiles, n_live);
}

int antsrl_memnet_dims(const char *who, const AntsMemNetShape *s, MemNetDims *d) { return memnet_check(s, d, who); }
int antsrl_memnet_precision(const char *who, int precision) { return memnet_precision(precision, who); }

// ---- the training step (antsrl_memtrain.hip)

// tensor i of the state_dict (weight, bias per layer) in the state's flat fp32 parameter block, in floats
struct ParamSpan {
    size_t off, n;
};
static ParamSpan param_span(const MemTrainLayout &L, int i)
{
    const int l = i / 2;
    const size_t w = (size_t)L.out[l] * L.in[l];
    return i % 2 ? ParamSpan{L.poff[l] + w, (size_t)L.out[l]} : ParamSpan{L.poff[l], w};
}

static int memtrain_state_check(const void *state, const char *who, const char *name)
{
    if (!state) return fail(ANTSRL_E_INVALID, "%s: %s is required", who, name);
    if ((uintptr_t)state & 255) return fail(ANTSRL_E_INVALID, "%s: %s must be 256-byte aligned", who, name);
    return ANTSRL_OK;
}

extern "C" int antsrl_memtrain_sizes(const AntsMemNetShape *s, int64_t B, size_t *params_floats, size_t *trained_floats,
                                     size_t *state_bytes, size_t *workspace_bytes)
{
    MemNetDims d;
    const int rc = memnet_check(s, &d, "memtrain_sizes");
    if (rc != ANTSRL_OK) return rc;
    if (B < 1 || B > MT_MAX_B) return fail(ANTSRL_E_INVALID, "memtrain_sizes: B must be in [1, 2^24]");
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    MemTrainWork W;
    antsrl_memtrain_work_layout(d, (int)B, &W);
    if (params_floats) *params_floats = L.params_floats;
    if (trained_floats) *trained_floats = L.trained_floats;
    if (state_bytes) *state_bytes = L.bytes;
    if (workspace_bytes) *workspace_bytes = W.bytes;
    return ANTSRL_OK;
}

extern "C" int antsrl_memtrain_init(const AntsMemNetShape *s, const float *const *params, void *state, void *stream)
{
    MemNetDims d;
    int rc = memnet_check(s, &d, "memtrain_init");
    if (rc != ANTSRL_OK) return rc;
    if (!params) return fail(ANTSRL_E_INVALID, "memtrain_init: params is required");
    if ((rc = check_params("memtrain_init", params)) != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(state, "memtrain_init", "state")) != ANTSRL_OK) return rc;
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *S = (unsigned char *)state;
    hipError_t e = hipMemsetAsync(S, 0, L.bytes, st); // m = v = 0, zero padding everywhere (the packs' included)
    for (int i = 0; i < 26 && e == hipSuccess; ++i) {
        const ParamSpan p = param_span(L, i);
        e = hipMemcpyAsync(S + p.off * 4, params[i], p.n * 4, hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = antsrl_launch_memtrain_repack(d, S, st);
    return enqueued(e, "memtrain_init");
}

extern "C" int antsrl_memtrain_unpack(const AntsMemNetShape *s, const void *state, float *const *params, void *stream)
{
    MemNetDims d;
    int rc = memnet_check(s, &d, "memtrain_unpack");
    if (rc != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(state, "memtrain_unpack", "state")) != ANTSRL_OK) return rc;
    if (!params) return fail(ANTSRL_E_INVALID, "memtrain_unpack: params is required");
    if ((rc = check_params("memtrain_unpack", params)) != ANTSRL_OK) return rc;
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    const unsigned char *S = (const unsigned char *)state;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 26 && e == hipSuccess; ++i) {
        const ParamSpan p = param_span(L, i);
        e = hipMemcpyAsync(params[i], S + p.off * 4, p.n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    }
    return enqueued(e, "memtrain_unpack");
}

extern "C" int antsrl_memtrain_copy(const AntsMemNetShape *s, const void *src_state, void *dst_state, void *stream)
{
    MemNetDims d;
    int rc = memnet_check(s, &d, "memtrain_copy");
    if (rc != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(src_state, "memtrain_copy", "src_state")) != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(dst_state, "memtrain_copy", "dst_state")) != ANTSRL_OK) return rc;
    MemTrainLayout L;
    antsrl_memtrain_state_layout(d, &L);
    const unsigned char *S = (const unsigned char *)src_state;
    unsigned char *T = (unsigned char *)dst_state;
    if (S == T) return ANTSRL_OK;
    hipError_t e = hipMemcpyAsync(T, S, L.params_floats * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(T + L.pack_off, S + L.pack_off, L.bytes - L.pack_off, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return enqueued(e, "memtrain_copy");
}

extern "C" int antsrl_memtrain_grad(const AntsMemNetShape *s, const void *state, const void *target_state,
                                    const float *states, const float *agent_states, const int64_t *actions,
                                    const float *rewards, const float *new_states, const float *new_agent_states,
                                    const uint8_t *dones, const int64_t *idx, int64_t B, float discount, float *grads,
                                    float *loss_out, void *workspace, void *stream)
{
    MemNetDims d;
    int rc = memnet_check(s, &d, "memtrain_grad");
    if (rc != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(state, "memtrain_grad", "state")) != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(target_state, "memtrain_grad", "target_state")) != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(workspace, "memtrain_grad", "workspace")) != ANTSRL_OK) return rc;
    if (!states || !agent_states || !actions || !rewards || !new_states || !new_agent_states || !dones)
        return fail(ANTSRL_E_INVALID, "memtrain_grad: states, agent_states, actions, rewards, new_states, new_agent_states, "
                                      "dones are required");
    if (!grads || !loss_out) return fail(ANTSRL_E_INVALID, "memtrain_grad: grads and loss_out are required");
    if (((uintptr_t)states | (uintptr_t)agent_states | (uintptr_t)new_states | (uintptr_t)new_agent_states |
         (uintptr_t)rewards | (uintptr_t)grads | (uintptr_t)loss_out) & 3)
        return fail(ANTSRL_E_INVALID, "memtrain_grad: float arrays must be 4-byte aligned");
    if (((uintptr_t)actions | (uintptr_t)idx) & 7)
        return fail(ANTSRL_E_INVALID, "memtrain_grad: actions and idx must be 8-byte aligned");
    if (B < 1 || B > MT_MAX_B) return fail(ANTSRL_E_INVALID, "memtrain_grad: B must be in [1, 2^24]");
    if (!(discount == discount)) return fail(ANTSRL_E_INVALID, "memtrain_grad: discount is NaN");
    const MemTrainBatch bt{states, agent_states, rewards, new_states, new_agent_states, actions, idx, dones};
    hipError_t e = antsrl_launch_memtrain_grad(d, (const unsigned char *)state, (const unsigned char *)target_state, bt,
                                               (int)B, discount, grads, loss_out, (unsigned char *)workspace,
                                               (hipStream_t)stream);
    return enqueued(e, "memtrain_grad");
}

extern "C" int antsrl_memtrain_apply(const AntsMemNetShape *s, void *state, const float *grads, int64_t step, double lr,
                                     double beta1, double beta2, double eps, void *stream)
{
    MemNetDims d;
    int rc = memnet_check(s, &d, "memtrain_apply");
    if (rc != ANTSRL_OK) return rc;
    if ((rc = memtrain_state_check(state, "memtrain_apply", "state")) != ANTSRL_OK) return rc;
    if (!grads) return fail(ANTSRL_E_INVALID, "memtrain_apply: grads is required");
    if ((uintptr_t)grads & 3) return fail(ANTSRL_E_INVALID, "memtrain_apply: grads must be 4-byte aligned");
    AdamArgs o = {};
    if ((rc = antsrl_adam_args("memtrain_apply", step, lr, beta1, beta2, eps, &o)) != ANTSRL_OK) return rc;
    hipError_t e = antsrl_launch_memtrain_apply(d, (unsigned char *)state, grads, o.step_size, o.bc2_sqrt, o.w1m, o.beta2,
                                                o.w2m, o.eps, (hipStream_t)stream);
    return enqueued(e, "memtrain_apply");
}
