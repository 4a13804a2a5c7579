// antsrl_explored.h — the EXPLORED SUMMARY of the cell-meta path, in ONE place: one bit per tile of 8 x 8 cells, kept in the
// environment's own slice of DState::explored_bits (dead space on that path: cell_explored() reads the META word there).
// Used by k_explored_summary / k_perceive (antsrl_perceive.hip) and by the host-side test (tests/test_explored_summary_cpu.py
// compiles this header with g++).
//
// CONTRACT.  A set bit means: every cell of the tile carried an explored stamp when the bit was set, and bits are only
// ever set BETWEEN observations — so every such cell was explored by an observation that had completed.  Exploredness is
// monotone within an episode (a stamp is never taken back; the stamp re-base keeps explored cells explored), so a bit stays
// true until the next reset, which clears the whole array.  A clear bit says nothing.
//
// What k_perceive does with it: an ant whose patch can only touch tiles with a set bit cannot count or mark an unexplored
// cell, so the records of its MASKED cells — gathered for that count alone — are not needed (explored_box_full below).
//
// Power-of-two grids of at least 8 x 8 cells only (k_perceive's fast path): explored_tiles_ok.  Anything else never sets a bit.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define EXPL_TILE_SHIFT 3 // 8 x 8 cells per tile: 4 x 4 tiles buy 1 % fewer gathered lines at c3 for four times the bits

__host__ __device__ inline bool explored_tiles_ok(const int W, const int H)
{
    return W >= (1 << EXPL_TILE_SHIFT) && H >= (1 << EXPL_TILE_SHIFT) && (W & (W - 1)) == 0 && (H & (H - 1)) == 0;
}

// tiles of the grid, and the summary bit of the tile of cell (x, y), 0 <= x < W, 0 <= y < H: tiles row-major over
// (x / 8, y / 8) like the cells of every canonical map — bit t lives in word t >> 5 at position t & 31
__host__ __device__ inline uint32_t explored_tile_count(const int W, const int H)
{
    return (uint32_t)(W >> EXPL_TILE_SHIFT) * (uint32_t)(H >> EXPL_TILE_SHIFT);
}
__host__ __device__ inline uint32_t explored_tile_index(const int x, const int y, const int H)
{
    return (uint32_t)((x >> EXPL_TILE_SHIFT) * (H >> EXPL_TILE_SHIFT) + (y >> EXPL_TILE_SHIFT));
}
__host__ __device__ inline uint32_t explored_tile_word(const uint32_t t) { return t >> 5; }
__host__ __device__ inline uint32_t explored_tile_bit(const uint32_t t) { return t & 31u; }

// The tiles the patch of one ant can touch.  A perceived cell is rint(c + d) per axis with |d| <= r * delta * sqrt(2) (the
// patch's corner, RL_api.py:110-117), i.e. an integer within `margin` = r * delta * sqrt(2) + 0.5 of the perception
// frame's centre c: all of them lie in [floor(c - margin), ceil(c + margin)], then wrapped (RL_api.py:118-119).  The box
// is kept unwrapped: first tile (may be negative) and number of tiles per axis, clipped to the whole axis.
struct ExplBox {
    int tx0, ntx, ty0, nty;
};

__host__ __device__ inline double explored_box_margin(const int r, const double delta)
{
    return (double)r * delta * 1.4142135623730951 + 0.5;
}

__host__ __device__ inline int expl_floor_i(const double v)
{
    const int i = (int)v;
    return (double)i > v ? i - 1 : i;
}
__host__ __device__ inline int expl_ceil_i(const double v)
{
    const int i = (int)v;
    return (double)i < v ? i + 1 : i;
}

__host__ __device__ inline ExplBox explored_box(const double cx, const double cy, const double margin, const int W, const int H)
{
    ExplBox b;
    const int tw = W >> EXPL_TILE_SHIFT, th = H >> EXPL_TILE_SHIFT;
    const int x0 = expl_floor_i(cx - margin) >> EXPL_TILE_SHIFT, x1 = expl_ceil_i(cx + margin) >> EXPL_TILE_SHIFT; // (arithmetic shift: floor)
    const int y0 = expl_floor_i(cy - margin) >> EXPL_TILE_SHIFT, y1 = expl_ceil_i(cy + margin) >> EXPL_TILE_SHIFT;
    b.tx0 = x0;
    b.ntx = x1 - x0 + 1 < tw ? x1 - x0 + 1 : tw;
    b.ty0 = y0;
    b.nty = y1 - y0 + 1 < th ? y1 - y0 + 1 : th;
    return b;
}

// The same verdict as explored_box_full below for a box of at most three tile columns and at most 32 tiles per column (the
// reference's patch: three by three at most), with every load in front of every use: a column's run of bits then lies in
// at most two words — cut once, by the wrap or by a word boundary (columns of fewer than 32 tiles never straddle a word,
// longer ones are whole words) — so six unconditional loads (a narrower box repeats its last column) and bit arithmetic.
// In explored_box_full every word waits for the one before it: three memory round trips in a row in front of a wave's
// first gather, where this form has one.
__host__ __device__ inline bool explored_box_small(const ExplBox b) { return b.ntx <= 3 && b.nty <= 32; }

__host__ __device__ inline bool explored_box_full_small(const uint32_t *bits, const ExplBox b, const int W, const int H)
{
    const int tw = W >> EXPL_TILE_SHIFT, th = H >> EXPL_TILE_SHIFT;
    const uint32_t t_first = (uint32_t)(b.ty0 & (th - 1)), t_last = (uint32_t)((b.ty0 + b.nty - 1) & (th - 1));
    uint32_t wa[3], wb[3], va[3], vb[3];
    for (int i = 0; i < 3; ++i) {
        const uint32_t base = (uint32_t)((b.tx0 + (i < b.ntx ? i : b.ntx - 1)) & (tw - 1)) * (uint32_t)th;
        wa[i] = explored_tile_word(base + t_first);
        wb[i] = explored_tile_word(base + t_last);
    }
    for (int i = 0; i < 3; ++i) {
        va[i] = bits[wa[i]];
        vb[i] = bits[wb[i]];
    }
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        const uint32_t base = (uint32_t)((b.tx0 + (i < b.ntx ? i : b.ntx - 1)) & (tw - 1)) * (uint32_t)th;
        uint32_t ma = 0u, mb = 0u;
        for (int j = 0; j < b.nty; ++j) {
            const uint32_t t = base + (uint32_t)((b.ty0 + j) & (th - 1)), m = 1u << explored_tile_bit(t);
            if (explored_tile_word(t) == wa[i]) ma |= m;
            else mb |= m;
        }
        ok = ok & ((va[i] & ma) == ma) & ((vb[i] & mb) == mb);
    }
    return ok;
}

// "All tiles of the box are set" against the environment's summary words.  Per tile column the box is one run of bits,
// cut where it wraps and at word boundaries: at 256 x 256 with the reference's 7 x 7 patch that is one word per column, three
// words of one 128-byte line per ant.  (No early exit: the loads do not wait for each other's verdict.)
__host__ __device__ inline bool explored_box_full(const uint32_t *bits, const ExplBox b, const int W, const int H)
{
    const int tw = W >> EXPL_TILE_SHIFT, th = H >> EXPL_TILE_SHIFT;
    bool ok = true;
    for (int i = 0; i < b.ntx; ++i) {
        const uint32_t base = (uint32_t)((b.tx0 + i) & (tw - 1)) * (uint32_t)th;
        int ty = b.ty0 & (th - 1), n = b.nty;
        while (n > 0) {
            const uint32_t t = base + (uint32_t)ty, pos = explored_tile_bit(t);
            int take = n;
            if (take > 32 - (int)pos) take = 32 - (int)pos;
            if (take > th - ty) take = th - ty;
            const uint32_t m = (take >= 32 ? ~0u : (1u << take) - 1u) << pos;
            const bool full = (bits[explored_tile_word(t)] & m) == m;
            ok = ok & full;
            ty = (ty + take) & (th - 1);
            n -= take;
        }
    }
    return ok;
}
