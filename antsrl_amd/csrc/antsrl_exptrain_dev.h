// antsrl_exptrain_dev.h — what the two kernels that run the forward stage of the explore agent's training step share
// around its body (antsrl_exptrain_fwd_body.inc): k_exptrain_fwd (antsrl_exptrain.hip: one net) and k_pop_exptrain_fwd
// (antsrl_popexplore.hip: one net per member of a population, the member taken from the grid).  Here are the body's LDS
// layout, its rounding helper and the size of its dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>
#include "antsrl_dqn_dev.h"
#include "antsrl_exptrain.h"

#define ET_HSTRIDE 33 // floats per row of a wave's h tile: 32 hidden values and the 1.0 of b2
#define ET_DSTRIDE 4  // floats per row of its dq tile: 3 dq, the loss term
#define ET_SLOT 100   // floats per layer2 in LDS: [3][32] + [3], padded to 16 bytes
#define ET_TILE (32 * ET_HSTRIDE + 32 * ET_DSTRIDE)

__device__ __forceinline__ float et_bf16(const float x) { return (float)(__bf16)x; }

// the forward stage's dynamic LDS: 61 KB at F = 294, 151 KB at the widest rows: above 64 KiB it is an opt-in per device
inline size_t ExpNet::lds(int ksteps)
{
    return (size_t)2 * ET_HIDDEN * (16 * ksteps + 8) * 2 +
           (2 * ET_SLOT + 6 * ET_HIDDEN + (size_t)ET_WAVES * ET_PART + (size_t)ET_WAVES * ET_TILE) * 4;
}
