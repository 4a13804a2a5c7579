// antsrl_logapi.hip — the device-resident logs' part of the C-ABI of libantsrl_hip.so (include/antsrl.h): the episode
// recorder (kernels in antsrl_recorder.hip), the colony statistics (antsrl_stats.hip) and the episode renderer, which takes
// the recorder's block and its layout (antsrl_render.hip).
//
// Host-side only: validates the arguments, enqueues the handle's deferred update where a log holds the state behind it
// (antsrl_handle.h), then the kernels on the caller's stream.  No allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "antsrl_handle.h"
#include "antsrl_recorder.h"
#include "antsrl_stats.h"
#include "antsrl_render.h"

// the configuration keeps an explored map (the heatmap of a recorded frame, explored_cells of a statistics row)
static bool keeps_map(const AntsHandle *h)
{
    return h->cfg.reward_kind == ANTSRL_REWARD_EXPLORATION || h->cfg.reward_kind == ANTSRL_REWARD_ALL;
}

// ---- the episode recorder (include/antsrl.h, "The episode recorder"; kernels in antsrl_recorder.hip) ------------------
static int recorder_layout(const char *who, const AntsHandle *h, int32_t n_sel, int32_t max_frames, int32_t with_heatmap,
                           RecorderLayout *L)
{
    if (!h) return fail(ANTSRL_E_INVALID, "%s: NULL handle", who);
    if (n_sel < 1 || n_sel > ANTSRL_RECORDER_MAX_ENVS)
        return fail(ANTSRL_E_INVALID, "%s: n_sel %d is not in 1..%d", who, n_sel, ANTSRL_RECORDER_MAX_ENVS);
    if (max_frames < 1) return fail(ANTSRL_E_INVALID, "%s: max_frames must be >= 1 (%d)", who, max_frames);
    *L = antsrl_recorder_layout(n_sel, h->p.N, h->p.R, h->p.C, (size_t)h->p.W * h->p.H, with_heatmap && keeps_map(h) ? 1 : 0);
    return ANTSRL_OK;
}

// every argument of _begin / _frame (has_frame), before any HIP call
static int recorder_check(const char *who, const AntsHandle *h, const void *block, const int32_t *env_indices, int32_t n_sel,
                          int32_t max_frames, int32_t with_heatmap, bool has_frame, int32_t frame, RecorderLayout *L, RecorderSel *sel)
{
    int rc = recorder_layout(who, h, n_sel, max_frames, with_heatmap, L);
    if (rc) return rc;
    if (!block) return fail(ANTSRL_E_INVALID, "%s: NULL block", who);
    if ((uintptr_t)block & 15) return fail(ANTSRL_E_INVALID, "%s: block must be 16-byte aligned", who);
    if (!env_indices) return fail(ANTSRL_E_INVALID, "%s: NULL env_indices", who);
    memset(sel, 0, sizeof(*sel));
    for (int s = 0; s < n_sel; ++s) {
        const int32_t e = env_indices[s];
        if (e < 0 || e >= h->p.E)
            return fail(ANTSRL_E_INVALID, "%s: env_indices[%d] = %d is not in [0, n_envs = %d)", who, s, e, h->p.E);
        for (int t = 0; t < s; ++t)
            if (sel->env[t] == e) return fail(ANTSRL_E_INVALID, "%s: env_indices[%d] repeats environment %d", who, s, e);
        sel->env[s] = e;
    }
    if (has_frame && (frame < 0 || frame >= max_frames))
        return fail(ANTSRL_E_INVALID, "%s: frame %d is not in [0, max_frames = %d)", who, frame, max_frames);
    return handle_ready(h, MID_UPDATE_REFUSED);
}

extern "C" int antsrl_recorder_sizes(const AntsHandle *h, int32_t n_sel, int32_t max_frames, int32_t with_heatmap,
                                     size_t *static_bytes, size_t *frame_bytes, size_t *bytes)
{
    RecorderLayout L;
    int rc = recorder_layout("recorder_sizes", h, n_sel, max_frames, with_heatmap, &L);
    if (rc) return rc;
    if (static_bytes) *static_bytes = L.static_bytes;
    if (frame_bytes) *frame_bytes = L.frame_bytes;
    if (bytes) *bytes = L.static_bytes + (size_t)max_frames * L.frame_bytes;
    return ANTSRL_OK;
}

extern "C" int antsrl_recorder_begin(AntsHandle *h, void *block, const int32_t *env_indices, int32_t n_sel,
                                     int32_t max_frames, int32_t with_heatmap, void *stream)
{
    RecorderLayout L;
    RecorderSel sel;
    int rc = recorder_check("recorder_begin", h, block, env_indices, n_sel, max_frames, with_heatmap, false, 0, &L, &sel);
    if (rc) return rc;
    rc = flush_pending(h, (hipStream_t)stream); // (as antsrl_read_state: the log holds the state after the update)
    if (rc) return rc;
    return enqueued(antsrl_launch_record_static(h->p, L, sel, (unsigned char *)block, (hipStream_t)stream), "recorder_begin");
}

extern "C" int antsrl_recorder_frame(AntsHandle *h, void *block, const int32_t *env_indices, int32_t n_sel,
                                     int32_t max_frames, int32_t with_heatmap, int32_t frame, void *stream)
{
    RecorderLayout L;
    RecorderSel sel;
    int rc = recorder_check("recorder_frame", h, block, env_indices, n_sel, max_frames, with_heatmap, true, frame, &L, &sel);
    if (rc) return rc;
    rc = flush_pending(h, (hipStream_t)stream); // a frame is the state AFTER Environment.update (main.py:138)
    if (rc) return rc;
    return enqueued(antsrl_launch_record_frame(h->p, h->cur, L, sel,
                                               (unsigned char *)block + L.static_bytes + (size_t)frame * L.frame_bytes,
                                               (hipStream_t)stream),
                    "recorder_frame");
}

// ---- the colony statistics (include/antsrl.h, "The colony statistics"; kernels in antsrl_stats.hip) -------------------
static int stats_layout(const char *who, const AntsHandle *h, int32_t max_rows, StatsLayout *L)
{
    if (!h) return fail(ANTSRL_E_INVALID, "%s: NULL handle", who);
    if (max_rows < 1) return fail(ANTSRL_E_INVALID, "%s: max_rows must be >= 1 (%d)", who, max_rows);
    *L = antsrl_stats_layout(h->p.E, h->p.C, (size_t)h->p.W * h->p.H, keeps_map(h) ? 1 : 0);
    return ANTSRL_OK;
}

extern "C" int antsrl_stats_sizes(const AntsHandle *h, int32_t max_rows, size_t *row_bytes, size_t *scratch_bytes, size_t *bytes)
{
    StatsLayout L;
    int rc = stats_layout("stats_sizes", h, max_rows, &L);
    if (rc) return rc;
    if (row_bytes) *row_bytes = 8 * L.row_words;
    if (scratch_bytes) *scratch_bytes = 8 * L.scratch_words;
    if (bytes) *bytes = 8 * ((size_t)max_rows * L.row_words + L.scratch_words);
    return ANTSRL_OK;
}

extern "C" int antsrl_stats_row(AntsHandle *h, void *block, int32_t max_rows, int32_t row, void *stream)
{
    const char *who = "stats_row";
    StatsLayout L;
    int rc = stats_layout(who, h, max_rows, &L);
    if (rc) return rc;
    if (!block) return fail(ANTSRL_E_INVALID, "%s: NULL block", who);
    if ((uintptr_t)block & 7) return fail(ANTSRL_E_INVALID, "%s: block must be 8-byte aligned", who);
    if (row < 0 || row >= max_rows) return fail(ANTSRL_E_INVALID, "%s: row %d is not in [0, max_rows = %d)", who, row, max_rows);
    rc = handle_ready(h, MID_UPDATE_REFUSED);
    if (rc) return rc;
    rc = flush_pending(h, (hipStream_t)stream); // a row is the state AFTER Environment.update, as a recorded frame is
    if (rc) return rc;
    double *words = (double *)block;
    return enqueued(antsrl_launch_stats_row(h->p, h->cur, L, words + (size_t)row * L.row_words,
                                            words + (size_t)max_rows * L.row_words, (hipStream_t)stream),
                    who);
}

// ---- the episode renderer (include/antsrl.h, "The episode renderer"; kernels in antsrl_render.hip) --------------------
static int render_opts(const char *who, const AntsHandle *h, int32_t n_sel, const AntsRenderOpts *o)
{
    if (!h) return fail(ANTSRL_E_INVALID, "%s: NULL handle", who);
    if (!o) return fail(ANTSRL_E_INVALID, "%s: NULL opts", who);
    if (n_sel < 1 || n_sel > ANTSRL_RECORDER_MAX_ENVS)
        return fail(ANTSRL_E_INVALID, "%s: n_sel %d is not in 1..%d", who, n_sel, ANTSRL_RECORDER_MAX_ENVS);
    if (o->zoom < 1 || o->zoom > ANTSRL_RENDER_MAX_ZOOM)
        return fail(ANTSRL_E_INVALID, "%s: zoom %d is not in 1..%d", who, o->zoom, ANTSRL_RENDER_MAX_ZOOM);
    if (o->ant_radius < 0 || o->ant_radius > ANTSRL_RENDER_MAX_ANT_RADIUS)
        return fail(ANTSRL_E_INVALID, "%s: ant_radius %d is not in 0..%d", who, o->ant_radius, ANTSRL_RENDER_MAX_ANT_RADIUS);
    if (!(o->phero_max_val > 0.0)) return fail(ANTSRL_E_INVALID, "%s: phero_max_val must be > 0 (%g)", who, o->phero_max_val);
    if (o->view_mask & ~ANTSRL_RENDER_VIEW_ALL)
        return fail(ANTSRL_E_INVALID, "%s: view_mask 0x%x has bits outside 0x%x", who, (unsigned)o->view_mask, ANTSRL_RENDER_VIEW_ALL);
    return ANTSRL_OK;
}

extern "C" int antsrl_render_sizes(const AntsHandle *h, int32_t n_sel, const AntsRenderOpts *o, size_t *frame_env_bytes,
                                   size_t *scratch_bytes_per_frame)
{
    int rc = render_opts("render_sizes", h, n_sel, o);
    if (rc) return rc;
    const size_t W = (size_t)h->p.W, H = (size_t)h->p.H, Z = (size_t)o->zoom;
    if (frame_env_bytes) *frame_env_bytes = o->layer_only ? 4 * W * H : 3 * (W * Z) * (H * Z);
    if (scratch_bytes_per_frame) *scratch_bytes_per_frame = 4 * (size_t)n_sel;
    return ANTSRL_OK;
}

extern "C" int antsrl_render_frames(AntsHandle *h, const void *block, int32_t n_sel, int32_t max_frames, int32_t with_heatmap,
                                    int32_t first, int32_t count, const AntsRenderOpts *o, void *out, void *scratch, void *stream)
{
    const char *who = "render_frames";
    int rc = render_opts(who, h, n_sel, o);
    if (rc) return rc;
    RenderArgs a;
    memset(&a, 0, sizeof(a));
    rc = recorder_layout(who, h, n_sel, max_frames, with_heatmap, &a.L);
    if (rc) return rc;
    if (!block) return fail(ANTSRL_E_INVALID, "%s: NULL block", who);
    if (!out) return fail(ANTSRL_E_INVALID, "%s: NULL out", who);
    if (!scratch) return fail(ANTSRL_E_INVALID, "%s: NULL scratch", who);
    if ((uintptr_t)block & 15) return fail(ANTSRL_E_INVALID, "%s: block must be 16-byte aligned", who);
    if ((uintptr_t)out & 15) return fail(ANTSRL_E_INVALID, "%s: out must be 16-byte aligned", who);
    if ((uintptr_t)scratch & 15) return fail(ANTSRL_E_INVALID, "%s: scratch must be 16-byte aligned", who);
    if (first < 0 || count < 1 || (long long)first + count > max_frames)
        return fail(ANTSRL_E_INVALID, "%s: frames %d .. %d + %d are not inside [0, max_frames = %d)", who, first, first, count, max_frames);
    const size_t groups = o->layer_only ? render_layer_groups(a.L.G) : render_tiles(h->p.W, h->p.H, o->zoom);
    if (count > 65535 || groups * (size_t)n_sel * (size_t)count >= ANTSRL_RENDER_MAX_GROUPS)
        return fail(ANTSRL_E_INVALID, "%s: count %d is past the launch limits (65535 frames, %zu workgroups per frame of 2^24): split the call",
                    who, count, groups * (size_t)n_sel);
    rc = handle_ready(h, MID_UPDATE_ALLOWED); // (the block was recorded from this handle; it reads no state)
    if (rc) return rc;
    a.block = (const unsigned char *)block;
    a.out = (unsigned char *)out;
    a.fmax = (int32_t *)scratch;
    a.W = h->p.W; a.H = h->p.H; a.Z = o->zoom; a.TY = render_ty(o->zoom); a.view = o->view_mask; a.ra = o->ant_radius; a.first = first; a.count = count;
    a.phero_den = o->phero_max_val + 0.0001;
    memcpy(a.col, o->phero_colors, sizeof(a.col));
    return enqueued(antsrl_launch_render(a, o->layer_only != 0, (hipStream_t)stream), who);
}
