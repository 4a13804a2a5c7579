// antsrl_adam.h — one element of torch.optim.Adam's single-tensor step in fp32, shared by the memory agent's apply stage
// (antsrl_memtrain.hip) and the linear agent's training step (antsrl_lintrain.hip).  The host computes
// step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) in double and rounds every scalar to float once
// (w1 = 1 - beta1, w2 = 1 - beta2), as the op does.
#pragma once
#include <hip/hip_runtime.h>

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
