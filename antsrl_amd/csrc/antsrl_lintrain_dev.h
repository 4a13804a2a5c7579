// antsrl_lintrain_dev.h — what the two kernels that run the linear agent's gradient stage share around its body: k_lintrain
// (antsrl_lintrain.hip: one net, gridDim.x workgroups) and k_pop_lintrain (antsrl_population.hip: one workgroup per
// member of a population, each the fused one-workgroup form on its member's net and ring slab).  The body is ONE text,
// antsrl_lintrain_body.inc, included inside both kernels; here are its LDS layout and the step's epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_dqn_dev.h"
#include "antsrl_lintrain.h"

#define LT_HSTRIDE 33 // floats per row of a wave's h tile: 32 hidden values and the 1.0 of the biases
#define LT_DSTRIDE 8  // floats per row of its dq tile: 6 dq, the loss term, pad
#define LT_SLOT 100   // floats per head in LDS: [3][32] + [3], padded to 16 bytes
#define LT_HW 304     // the three slots, padded

// the stage's dynamic LDS for nw waves per workgroup
static inline size_t lt_lds(int ksteps, int nw)
{
    return (size_t)LT_HIDDEN * (16 * ksteps + 8) * 2 +
           (LT_HW + 3 * LT_HIDDEN + (size_t)nw * LT_PART + (size_t)nw * (32 * LT_HSTRIDE + 32 * LT_DSTRIDE)) * 4;
}

// what thread t < LT_OUT does with total t of the step: gradient t (and Adam on trained float t), or the loss
__device__ __forceinline__ void lt_epilogue(const LinTrainArgs &a, const int t, const float total)
{
    if (t == LT_HEADS)
        *a.batch.loss = total;
    else
        dqn_store_adam(a.heads, a.batch.grads, a.adam, t, total);
}
