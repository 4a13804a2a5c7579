// antsrl_cellread.h — one canonical cell's value out of whatever layout the handle keeps it in: the per-cell loads of
// k_read_state (antsrl_state.hip), of the episode recorder (antsrl_recorder.hip) and of the colony statistics
// (antsrl_stats.hip), in ONE place, so that a recorded frame, a statistics row and a state read-out cannot drift apart.
// `g` is the canonical (row-major) cell id x * H + y of environment `e`, G = W * H.
#pragma once
#include "antsrl_util.h"

// ANTSRL_S_PHERO / ANTSRL_S_PHERO_C*: channel c of phero[cur] — interleaved or separate records (KP::ps), tiled or row-major
// (prec_cell); scaled units are materialised (phero_now: v * g_now, below the threshold -> 0), as the perception gather does
__device__ __forceinline__ float phero_now(const KP &p, float v)
{
    if (p.scaled) {
        v *= (float)p.g_now;
        if (v < (float)p.threshold) v = 0.0f;
    }
    return v;
}
__device__ __forceinline__ float cell_phero(const KP &p, const int cur, const size_t e, const size_t G, const uint32_t g, const int c)
{
    return phero_now(p, p.s.phero[cur][(e * G + prec_cell(p, g)) * p.ps + c]);
}

// ANTSRL_S_FOOD: the food value of the cell's record (KP::fs, frec_cell)
__device__ __forceinline__ float cell_food(const KP &p, const size_t e, const size_t G, const uint32_t g)
{
    return p.s.food[(e * G + frec_cell(p, g)) * p.fs];
}

// ANTSRL_S_EXPLORED: cell-meta layout: explored <=> the cell carries a stamp; else k_act's bit map
__device__ __forceinline__ uint8_t meta_explored(const uint32_t meta) { return (uint8_t)((meta >> META_STAMP_SHIFT) != META_NEVER); }
__device__ __forceinline__ uint8_t cell_explored(const KP &p, const size_t e, const size_t G, const uint32_t g)
{
    if (p.meta) {
        const uint32_t *m = reinterpret_cast<const uint32_t *>(p.s.food) + 1;
        return meta_explored(m[(e * G + frec_cell(p, g)) * p.fs]);
    }
    return (uint8_t)test_bit(p.s.explored_bits + e * p.words, g);
}

// Every value of one cell, for a reader that wants them all (the colony statistics): cell_phero for the channels 0 .. C - 1,
// cell_food and, with `explored`, cell_explored.  INTER: the handle keeps the interleaved 16-byte {p0, p1, food, META / pad}
// records (KP::ps == 4 && KP::fs == 4, two channels; prec_cell == frec_cell there) — the record is then loaded ONCE, 16
// bytes, instead of once per quantity; cell_record is that load and cell_all_of its reading, apart, so that a reader can
// have the loads of several cells in flight before it reads the first.
struct CellAll {
    float ph[ANTSRL_MAX_PHERO], food;
    uint8_t explored;
};
__device__ __forceinline__ float4 cell_record(const KP &p, const int cur, const size_t e, const size_t G, const uint32_t g)
{
    return reinterpret_cast<const float4 *>(p.s.phero[cur])[e * G + prec_cell(p, g)];
}
__device__ __forceinline__ CellAll cell_all_of(const KP &p, const float4 &r, const size_t e, const uint32_t g, const bool explored)
{
    CellAll v;
    v.ph[0] = phero_now(p, r.x); v.ph[1] = phero_now(p, r.y); v.ph[2] = v.ph[3] = 0.0f;
    v.food = r.z;
    v.explored = 0;
    if (explored) v.explored = p.meta ? meta_explored(__float_as_uint(r.w)) : (uint8_t)test_bit(p.s.explored_bits + e * p.words, g);
    return v;
}
template <bool INTER>
__device__ __forceinline__ CellAll cell_all(const KP &p, const int cur, const size_t e, const size_t G, const uint32_t g, const bool explored)
{
    CellAll v;
    v.explored = 0;
    if (INTER) {
        v = cell_all_of(p, cell_record(p, cur, e, G, g), e, g, explored);
    } else {
#pragma unroll
        for (int c = 0; c < ANTSRL_MAX_PHERO; ++c) v.ph[c] = c < p.C ? cell_phero(p, cur, e, G, g, c) : 0.0f;
        v.food = cell_food(p, e, G, g);
        if (explored) v.explored = cell_explored(p, e, G, g);
    }
    return v;
}

// ANTSRL_S_WALLS / ANTSRL_S_ANTHILL_AREA (and the explored map of k_act): one bit of an environment's bit map
__device__ __forceinline__ uint8_t cell_bit(const KP &p, const uint32_t *bits, const size_t e, const uint32_t g)
{
    return (uint8_t)test_bit(bits + e * p.words, g);
}
