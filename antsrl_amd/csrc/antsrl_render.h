// antsrl_render.h — the episode renderer (antsrl_render.hip; include/antsrl.h, "The episode renderer", is the
// specification): what its kernels take, the tile they work on and the colours of the composition.  The kernels read the
// episode recorder's block (antsrl_recorder.h: the layout comes from antsrl_recorder_layout, nothing is restated here) and
// nothing else; the block is read-only to them.
//
// The viewer's options travel as AntsRenderOpts (include/antsrl.h); RenderArgs is what a launch carries by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "antsrl_device.h"
#include "antsrl_fail.h"
#include "antsrl_recorder.h"

// ---- the composition's colours (the header's text names the same values)
#define ANTSRL_RENDER_DIRT_R 134        // the background under view bit 0
#define ANTSRL_RENDER_DIRT_G 96
#define ANTSRL_RENDER_DIRT_B 67
#define ANTSRL_RENDER_WALL_R 96         // a wall cell ("rock" texture of the viewer), opaque
#define ANTSRL_RENDER_WALL_G 96
#define ANTSRL_RENDER_WALL_B 96
#define ANTSRL_RENDER_ROCK_R 150        // a rock's disc
#define ANTSRL_RENDER_ROCK_G 150
#define ANTSRL_RENDER_ROCK_B 150
#define ANTSRL_RENDER_ANTHILL_ALPHA 128 // ANTHILL_COLOR (0, 0, 255, 128)

// ---- the tile of k_render_frames: one workgroup takes TX x TY cells, TX * Z x TY * Z pixels, 4 bytes of LDS per pixel
// (the ants' owner tile, then the pixel's colour) and 4 per cell.  TX is the long side: a tile's row of pixels is
// 3 * TX * Z contiguous bytes.  TY falls with the zoom (render_ty), so that a workgroup's fixed work — its scan of all N
// ants, its barriers — is spread over some thousands of pixels at every zoom while the LDS stays at 32.5 KiB or less
// (at ANTSRL_RENDER_MAX_ZOOM): at least four workgroups per CU of 160 KiB.
#define ANTSRL_RENDER_TX 32
#define ANTSRL_RENDER_THREADS 256
static inline int render_ty(int Z) { return Z <= 2 ? 32 : Z == 3 ? 16 : Z <= 5 ? 8 : 4; }
// a launch: grid (tiles, S, count), bounded by 65535 in z and by tiles * S * count < 2^24 workgroups (2^32 threads)
#define ANTSRL_RENDER_MAX_GROUPS ((size_t)1 << 24)

struct RenderArgs {
    RecorderLayout L;
    const unsigned char *block; // the recorder's block (static part first)
    unsigned char *out;
    int32_t *fmax;              // scratch: [count][S] the food plane's maximum
    int W, H, Z, TY, view, ra, first, count;
    double phero_den;           // phero_max_val + 0.0001
    uint8_t col[ANTSRL_MAX_PHERO][3];
};

static inline size_t render_tiles(int W, int H, int Z)
{
    const int TY = render_ty(Z);
    return (size_t)((W + ANTSRL_RENDER_TX - 1) / ANTSRL_RENDER_TX) * (size_t)((H + TY - 1) / TY);
}
static inline size_t render_layer_groups(size_t G) { return (G + ANTSRL_RENDER_THREADS - 1) / ANTSRL_RENDER_THREADS; }

// the food maximum pre-pass, then the frames (layer_only: the colour layer as RGBA per cell)
ANTSRL_INTERNAL hipError_t antsrl_launch_render(const RenderArgs &a, int layer_only, hipStream_t st);
