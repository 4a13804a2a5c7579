// Host-side window onto antsrl_amd/csrc/antsrl_explored.h for tests/test_explored_summary_cpu.py: the SAME inline functions
// k_explored_summary and k_perceive use, behind a C interface.
#include "../../antsrl_amd/csrc/antsrl_explored.h"

extern "C" {

int expl_tiles_ok(int W, int H) { return explored_tiles_ok(W, H) ? 1 : 0; }
unsigned expl_tile_count(int W, int H) { return explored_tile_count(W, H); }
unsigned expl_tile_index(int x, int y, int H) { return explored_tile_index(x, y, H); }
unsigned expl_tile_word(unsigned t) { return explored_tile_word(t); }
unsigned expl_tile_bit(unsigned t) { return explored_tile_bit(t); }
double expl_box_margin(int r, double delta) { return explored_box_margin(r, delta); }

// out[4] = {tx0, ntx, ty0, nty}
void expl_box(double cx, double cy, double margin, int W, int H, int *out)
{
    const ExplBox b = explored_box(cx, cy, margin, W, H);
    out[0] = b.tx0; out[1] = b.ntx; out[2] = b.ty0; out[3] = b.nty;
}

int expl_box_full(const unsigned *bits, double cx, double cy, double margin, int W, int H)
{
    return explored_box_full(bits, explored_box(cx, cy, margin, W, H), W, H) ? 1 : 0;
}

// For n poses: is the box full against `bits` (out_full[i]), and does the box's tile set contain the tile of every one of
// the pose's `m` cells (cells: [n][m][2] wrapped integer coordinates)?  Returns the number of cells outside their box, plus
// 2^40 for every pose whose small-box form (explored_box_full_small, what k_perceive runs at the reference's sizes)
// disagrees with the general one; *n_small counts the poses that took the small form.
long expl_check_poses(const unsigned *bits, const double *cxy, const int *cells, long n, int m, double margin, int W, int H,
                      unsigned char *out_full, long *n_small)
{
    *n_small = 0;
    const int tw = W >> EXPL_TILE_SHIFT, th = H >> EXPL_TILE_SHIFT;
    long bad = 0;
    for (long i = 0; i < n; ++i) {
        const ExplBox b = explored_box(cxy[2 * i], cxy[2 * i + 1], margin, W, H);
        out_full[i] = explored_box_full(bits, b, W, H) ? 1 : 0;
        if (explored_box_small(b)) {
            *n_small += 1;
            if ((explored_box_full_small(bits, b, W, H) ? 1 : 0) != out_full[i]) bad += 1l << 40;
        }
        for (int c = 0; c < m; ++c) {
            const int tx = cells[(i * m + c) * 2] >> EXPL_TILE_SHIFT, ty = cells[(i * m + c) * 2 + 1] >> EXPL_TILE_SHIFT;
            bool in_x = false, in_y = false;
            for (int k = 0; k < b.ntx; ++k) in_x |= ((b.tx0 + k) & (tw - 1)) == tx;
            for (int k = 0; k < b.nty; ++k) in_y |= ((b.ty0 + k) & (th - 1)) == ty;
            bad += !(in_x && in_y);
        }
    }
    return bad;
}
}
