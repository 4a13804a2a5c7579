// antsrl_cellread.h — one canonical cell's value out of whatever layout the handle keeps it in: the per-cell loads of
// k_read_state (antsrl_state.hip) and of the episode recorder (antsrl_recorder.hip), in ONE place, so that a recorded
// frame and a state read-out cannot drift apart.  `g` is the canonical (row-major) cell id x * H + y of environment `e`,
// G = W * H.
#pragma once
#include "antsrl_util.h"

// ANTSRL_S_PHERO / ANTSRL_S_PHERO_C*: channel c of phero[cur] — interleaved or separate records (KP::ps), tiled or row-major
// (prec_cell); scaled units are materialised (v * g_now, below the threshold -> 0), as the perception gather does
__device__ __forceinline__ float cell_phero(const KP &p, const int cur, const size_t e, const size_t G, const uint32_t g, const int c)
{
    float v = p.s.phero[cur][(e * G + prec_cell(p, g)) * p.ps + c];
    if (p.scaled) {
        v *= (float)p.g_now;
        if (v < (float)p.threshold) v = 0.0f;
    }
    return v;
}

// ANTSRL_S_FOOD: the food value of the cell's record (KP::fs, frec_cell)
__device__ __forceinline__ float cell_food(const KP &p, const size_t e, const size_t G, const uint32_t g)
{
    return p.s.food[(e * G + frec_cell(p, g)) * p.fs];
}

// ANTSRL_S_EXPLORED: cell-meta layout: explored <=> the cell carries a stamp; else k_act's bit map
__device__ __forceinline__ uint8_t cell_explored(const KP &p, const size_t e, const size_t G, const uint32_t g)
{
    if (p.meta) {
        const uint32_t *m = reinterpret_cast<const uint32_t *>(p.s.food) + 1;
        return (uint8_t)((m[(e * G + frec_cell(p, g)) * p.fs] >> META_STAMP_SHIFT) != META_NEVER);
    }
    return (uint8_t)test_bit(p.s.explored_bits + e * p.words, g);
}

// ANTSRL_S_WALLS / ANTSRL_S_ANTHILL_AREA (and the explored map of k_act): one bit of an environment's bit map
__device__ __forceinline__ uint8_t cell_bit(const KP &p, const uint32_t *bits, const size_t e, const uint32_t g)
{
    return (uint8_t)test_bit(bits + e * p.words, g);
}
