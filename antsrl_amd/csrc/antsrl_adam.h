// antsrl_adam.h — torch.optim.Adam's single-tensor step in fp32, for the memory agent's apply stage (antsrl_memtrain.hip),
// the linear agent's training step (antsrl_lintrain.hip), the explore agent's (antsrl_exptrain.hip) and the rework
// agent's (antsrl_reworktrain.hip): the host side (antsrl_adam_args: the checks of an entry's Adam arguments and the
// scalars; antsrl_adam_step: a fused _step entry's moments and scalars; antsrl_adam_apply: antsrl_lintrain_apply /
// antsrl_exptrain_apply / antsrl_reworktrain_apply behind the net's own check), one element on the device (adam_element, adam_at) and the flat kernel (antsrl_launch_adam).  The host
// computes step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) in double and rounds every scalar to
// float once (w1m = 1 - beta1, w2m = 1 - beta2), as the op does.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/antsrl.h"
#include "antsrl_fail.h"

struct AdamArgs {
    int on;      // 0: no Adam step (gradients and loss only)
    float *m, *v; // Adam's moments, laid out as the parameters
    float step_size, bc2_sqrt, w1m, beta2, w2m, eps;
};

// an entry's step, lr, beta1, beta2, eps -> the scalars of *o (and o->on = 1), or the refusal
static inline int antsrl_adam_args(const char *who, int64_t step, double lr, double beta1, double beta2, double eps,
                                   AdamArgs *o)
{
    if (step < 1) return fail(ANTSRL_E_INVALID, "%s: step must be >= 1", who);
    if (!(lr >= 0.0) || !(lr < 1e30)) return fail(ANTSRL_E_INVALID, "%s: lr must be finite and >= 0", who);
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(ANTSRL_E_INVALID, "%s: beta1, beta2 must be in [0, 1)", who);
    if (!(eps > 0.0) || !(eps < 1e30)) return fail(ANTSRL_E_INVALID, "%s: eps must be finite and > 0", who);
    // torch.optim.Adam (single tensor): the bias corrections in double, then every scalar rounded to float by the op
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    o->on = 1;
    o->step_size = (float)(lr / bc1);
    o->bc2_sqrt = (float)pow(bc2, 0.5);
    o->w1m = (float)(1.0 - beta1);
    o->beta2 = (float)beta2;
    o->w2m = (float)(1.0 - beta2);
    o->eps = (float)eps;
    return ANTSRL_OK;
}

// Adam's part of a fused _step entry, behind its minibatch: the two moments, then antsrl_adam_args, into *o
static inline int antsrl_adam_step(const char *who, float *adam_m, float *adam_v, int64_t step, double lr, double beta1,
                                   double beta2, double eps, AdamArgs *o)
{
    REQUIRE(adam_m, 4);
    REQUIRE(adam_v, 4);
    o->m = adam_m; o->v = adam_v;
    return antsrl_adam_args(who, step, lr, beta1, beta2, eps, o);
}

// Adam on params[0 .. P) from grads (o.m, o.v and the scalars are read): one flat kernel, antsrl_lintrain.hip holds it
ANTSRL_INTERNAL hipError_t antsrl_launch_adam(float *params, const AdamArgs &o, const float *grads, int P, hipStream_t st);

// the rest of an _apply entry over a flat block of P floats, behind the entry's check of `params`
static inline int antsrl_adam_apply(const char *who, float *params, float *adam_m, float *adam_v, const float *grads,
                                    int64_t step, double lr, double beta1, double beta2, double eps, int P, void *stream)
{
    REQUIRE(adam_m, 4);
    REQUIRE(adam_v, 4);
    REQUIRE(grads, 4);
    AdamArgs o = {};
    const int rc = antsrl_adam_args(who, step, lr, beta1, beta2, eps, &o);
    if (rc != ANTSRL_OK) return rc;
    o.m = adam_m; o.v = adam_v;
    return enqueued(antsrl_launch_adam(params, o, grads, P, (hipStream_t)stream), who);
}

// returns the new parameter; mm and vv are Adam's moments of the element, updated in place
__device__ __forceinline__ float adam_element(float p, const float g, float &mm, float &vv, const float step_size,
                                              const float bc2_sqrt, const float w1, const float beta2, const float w2,
                                              const float eps)
{
    mm = mm + w1 * (g - mm);                        // exp_avg.lerp_(grad, 1 - beta1)
    vv = vv * beta2 + w2 * g * g;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(vv) / bc2_sqrt + eps; // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    return p + -step_size * (mm / denom);           // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// the step on element i of params from its gradient g
__device__ __forceinline__ void adam_at(float *params, const AdamArgs &o, const size_t i, const float g)
{
    float mm = o.m[i], vv = o.v[i];
    params[i] = adam_element(params[i], g, mm, vv, o.step_size, o.bc2_sqrt, o.w1m, o.beta2, o.w2m, o.eps);
    o.m[i] = mm;
    o.v[i] = vv;
}
