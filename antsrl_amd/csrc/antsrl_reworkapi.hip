// antsrl_reworkapi.hip — the rework agent's part of the C-ABI of libantsrl_hip.so (include/antsrl.h, "The rework agent's
// net"): antsrl_rework_collapsed_bytes, antsrl_rework_collapse and antsrl_policy_rework in front of antsrl_rework.hip's
// two kernels.
//
// Host-side only: validates every argument before any HIP call and enqueues one kernel on the caller's stream.  No
// handle, no allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antsrl_device.h"
#include "antsrl_fail.h"
#include "antsrl_rework.h"

static int enqueued(hipError_t e, const char *who) { return e != hipSuccess ? hip_fail(e, who) : ANTSRL_OK; }

static int rework_check(const AntsReworkShape *s, ReworkDims *d, const char *who)
{
    if (!s) return fail(ANTSRL_E_INVALID, "%s: NULL shape", who);
    const int32_t hidden[7] = {s->g1, s->g2, s->g3, s->r1, s->r2, s->r3, s->p1};
    static const char *const names[7] = {"g1", "g2", "g3", "r1", "r2", "r3", "p1"};
    if (s->n_features < 1 || s->agent_dim < 1 || s->n_rot < 1 || s->n_ph < 1)
        return fail(ANTSRL_E_INVALID, "%s: n_features, agent_dim, n_rot, n_ph must be >= 1", who);
    for (int i = 0; i < 7; ++i)
        if (hidden[i] < 1) return fail(ANTSRL_E_INVALID, "%s: %s must be >= 1 (%d)", who, names[i], hidden[i]);
    if (s->agent_dim != 2) return fail(ANTSRL_E_UNSUPPORTED, "%s: agent_dim %d is not 2", who, s->agent_dim);
    const long long D = (long long)s->n_features + s->agent_dim;
    if (D > RW_MAX_D) return fail(ANTSRL_E_UNSUPPORTED, "%s: D = n_features + agent_dim = %lld > %d", who, D, RW_MAX_D);
    for (int i = 0; i < 7; ++i)
        if (hidden[i] > RW_MAX_H) return fail(ANTSRL_E_UNSUPPORTED, "%s: %s %d > %d", who, names[i], hidden[i], RW_MAX_H);
    if (s->n_rot > RW_MAX_HEAD || s->n_ph > RW_MAX_HEAD)
        return fail(ANTSRL_E_UNSUPPORTED, "%s: n_rot, n_ph (%d, %d) must be <= %d", who, s->n_rot, s->n_ph, RW_MAX_HEAD);
    *d = ReworkDims{s->n_features, (int)D, s->g1, s->g2, s->g3, s->r1, s->r2, s->r3, s->p1, s->n_rot, s->n_ph};
    return ANTSRL_OK;
}

extern "C" int antsrl_rework_collapsed_bytes(const AntsReworkShape *s, size_t *bytes)
{
    const char *who = "rework_collapsed_bytes";
    ReworkDims d;
    const int rc = rework_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!bytes) return fail(ANTSRL_E_INVALID, "%s: NULL bytes", who);
    *bytes = sizeof(float) * ((size_t)(d.n_rot + d.n_ph) * d.D + (size_t)(d.n_rot + d.n_ph));
    return ANTSRL_OK;
}

extern "C" int antsrl_rework_collapse(const AntsReworkShape *s, const float *const *params, void *collapsed, void *stream)
{
    const char *who = "rework_collapse";
    ReworkDims d;
    const int rc = rework_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!params || !collapsed) return fail(ANTSRL_E_INVALID, "%s: params and collapsed are required", who);
    if ((uintptr_t)collapsed & 3) return fail(ANTSRL_E_INVALID, "%s: collapsed must be 4-byte aligned", who);
    ReworkParams P;
    for (int i = 0; i < 2 * RW_LAYERS; ++i) {
        if (!params[i]) return fail(ANTSRL_E_INVALID, "%s: params[%d] is NULL", who, i);
        if ((uintptr_t)params[i] & 3) return fail(ANTSRL_E_INVALID, "%s: params[%d] must be 4-byte aligned", who, i);
        P.p[i] = params[i];
    }
    return enqueued(antsrl_launch_rework_collapse(P, d, (float *)collapsed, (hipStream_t)stream), who);
}

extern "C" int antsrl_policy_rework(const AntsReworkShape *s, const void *collapsed, const void *obs, int obs_format,
                                    const float *agent_state, int64_t n_ants, int8_t *rotation, int8_t *pheromone,
                                    float *q_out, void *stream)
{
    const char *who = "policy_rework";
    ReworkDims d;
    const int rc = rework_check(s, &d, who);
    if (rc != ANTSRL_OK) return rc;
    if (!collapsed || !obs || !agent_state || !rotation || !pheromone)
        return fail(ANTSRL_E_INVALID, "%s: collapsed, obs, agent_state, rotation, pheromone are required", who);
    if (((uintptr_t)collapsed | (uintptr_t)obs | (uintptr_t)agent_state | (uintptr_t)q_out) & 3)
        return fail(ANTSRL_E_INVALID, "%s: collapsed, obs, agent_state and q_out must be 4-byte aligned", who);
    if (obs_format != ANTSRL_OBS_F32 && obs_format != ANTSRL_OBS_BF16)
        return fail(ANTSRL_E_INVALID, "%s: obs_format must be ANTSRL_OBS_F32 or ANTSRL_OBS_BF16", who);
    if (n_ants < 0 || n_ants > 0x7fffffff) return fail(ANTSRL_E_INVALID, "%s: n_ants must be in [0, 2^31)", who);
    if (n_ants == 0) return ANTSRL_OK; // nothing to do, nothing launched
    return enqueued(antsrl_launch_rework_act((const float *)collapsed, d, obs, obs_format == ANTSRL_OBS_BF16, agent_state,
                                             (int)n_ants, rotation, pheromone, q_out, (hipStream_t)stream),
                    who);
}
