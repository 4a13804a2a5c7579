// antsrl_reworkapi.h — the shape check of the rework net's C-ABI entries, shared by the single agent's
// (antsrl_reworkapi.hip) and the population's (antsrl_popapi.hip).  Host only.
#pragma once
#include <stdint.h>
#include "antsrl_fail.h"
#include "antsrl_rework.h"

// every rule of an AntsReworkShape, in the entries' words; fills *d
static inline int rework_check(const AntsReworkShape *s, ReworkDims *d, const char *who)
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
