// antsrl_jointtrain_dev.h — what the two kernels that run the forward stage of the joint training step share around its
// body (antsrl_jointtrain_fwd_body.inc): k_jointtrain_fwd (antsrl_jointtrain.hip: one net) and k_pop_jointtrain_fwd
// (antsrl_popjoint.hip: one net per member of a population, the member taken from the grid).  Here are the body's LDS
// layout and the size of its dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>
#include "antsrl_dqn_dev.h"
#include "antsrl_jointtrain.h"

#define JT_HSTRIDE 33 // floats per row of a wave's h tile: 32 hidden values and the 1.0 of the biases
#define JT_DSTRIDE 8  // floats per row of its dq tile: 6 dq, the loss term, pad
#define JT_SLOT 100   // floats per head in LDS: [3][32] + [3], padded to 16 bytes
#define JT_HW 304     // the three slots (layer2, layer3, the target's layer3), padded
#define JT_TILE (32 * JT_HSTRIDE + 32 * JT_DSTRIDE)

// the forward stage's dynamic LDS: 45 760 bytes at F = 294, 91 840 at the widest rows: above 64 KiB it is an opt-in per device
inline size_t JointNet::lds(int ksteps)
{
    return (size_t)JT_HIDDEN * (16 * ksteps + 8) * 2 +
           (JT_HW + 3 * JT_HIDDEN + (size_t)JT_WAVES * JT_PART + (size_t)JT_WAVES * JT_TILE) * 4;
}
