// antsrl_capi.hip — the environment's part of the C-ABI of libantsrl_hip.so (include/antsrl.h), the library's error
// reporting (antsrl_fail.h) and the handle's helpers (antsrl_handle.h).  The memory agent's net has its entries in
// antsrl_memapi.hip, the agents' loop in antsrl_loopapi.hip; the episode recorder's, the colony statistics' and the
// episode renderer's are in antsrl_logapi.hip.
//
// Host-side only: validates the configuration, carves the caller's device workspace into the
// state arrays of antsrl_device.h, and enqueues the kernels of antsrl_act / _update / _sweep / _state.hip on the
// caller's stream (antsrl_launch.h).  No allocation, no synchronisation, no exceptions across the ABI.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <new>

#include <stddef.h>

#include "antsrl_checkpoint.h"
#include "antsrl_handle.h"
#include "antsrl_launch.h"

static thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    return fail(ANTSRL_E_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

extern "C" int antsrl_abi_version(void) { return ANTSRL_ABI_VERSION; }
extern "C" size_t antsrl_cfg_size(void) { return sizeof(AntsCfg); }
extern "C" const char *antsrl_last_error(void) { return g_err; }

static void fill_kp(const AntsCfg *c, KP *p);

static int validate(const AntsCfg *c)
{
    if (!c) return fail(ANTSRL_E_INVALID, "cfg is NULL");
    if (c->abi_version != ANTSRL_ABI_VERSION)
        return fail(ANTSRL_E_INVALID, "AntsCfg.abi_version %d != library %d", c->abi_version, ANTSRL_ABI_VERSION);
    if (c->n_envs < 1 || c->n_ants < 1 || c->w < 1 || c->h < 1)
        return fail(ANTSRL_E_INVALID, "n_envs, n_ants, w, h must be >= 1");
    if ((long long)c->w * c->h > (1ll << 30)) return fail(ANTSRL_E_INVALID, "grid too large");
    if (c->n_envs > 65535) // the sweep / stencil kernels index envs with blockIdx.y
        return fail(ANTSRL_E_INVALID, "n_envs must be <= 65535 per handle (shard larger batches over handles / GPUs)");
    if (c->n_phero < 1 || c->n_phero > ANTSRL_MAX_PHERO)
        return fail(ANTSRL_E_INVALID, "n_phero must be in 1..%d", ANTSRL_MAX_PHERO);
    if (c->n_rocks < 0 || c->n_rocks > 32) return fail(ANTSRL_E_INVALID, "n_rocks must be in 0..32");
    if (c->perception_radius < 0 || 2 * c->perception_radius + 1 > ANTSRL_MAX_PSIDE)
        return fail(ANTSRL_E_INVALID, "perception side must be <= %d", ANTSRL_MAX_PSIDE);
    if (c->n_channels < 1 || c->n_channels > ANTSRL_MAX_CHANNELS)
        return fail(ANTSRL_E_INVALID, "n_channels must be in 1..%d", ANTSRL_MAX_CHANNELS);
    for (int k = 0; k < c->n_channels; ++k) {
        const int kind = c->channel_kind[k];
        if (kind < ANTSRL_CH_ANTS || kind > ANTSRL_CH_ROCKS) return fail(ANTSRL_E_INVALID, "bad channel kind");
        if (kind == ANTSRL_CH_PHERO && (c->channel_arg[k] < 0 || c->channel_arg[k] >= c->n_phero))
            return fail(ANTSRL_E_INVALID, "pheromone channel index out of range");
        if (kind == ANTSRL_CH_PHERO && !c->has_max_val) // phero / None raises TypeError, RL_api.py:125
            return fail(ANTSRL_E_INVALID, "a perceived pheromone needs max_val (RL_api.py:125 divides by it)");
        if (kind == ANTSRL_CH_ROCKS && c->n_rocks == 0)
            return fail(ANTSRL_E_INVALID, "rocks perceived but n_rocks == 0");
    }
    if (c->filter_radius < 0 || c->filter_radius > ANTSRL_MAX_FILTER_RADIUS)
        return fail(ANTSRL_E_INVALID, "filter_radius must be in 0..%d", ANTSRL_MAX_FILTER_RADIUS);
    if (c->reward_kind < ANTSRL_REWARD_NONE || c->reward_kind > ANTSRL_REWARD_ALL)
        return fail(ANTSRL_E_INVALID, "bad reward_kind");
    if (c->has_max_val && !(c->phero_max_val > 0)) return fail(ANTSRL_E_INVALID, "phero_max_val must be > 0");
    if (c->act_path < ANTSRL_ACT_AUTO || c->act_path > ANTSRL_ACT_SINGLE_KERNEL) return fail(ANTSRL_E_INVALID, "bad act_path");
    if (c->env_id_base < 0 || (long long)c->env_id_base + c->n_envs > 0x7fffffffll)
        return fail(ANTSRL_E_INVALID, "env_id_base must be >= 0 and env_id_base + n_envs must fit 31 bits");
    if (c->n_envs_total != 0 && (long long)c->n_envs_total < (long long)c->env_id_base + c->n_envs)
        return fail(ANTSRL_E_INVALID, "n_envs_total %d < env_id_base + n_envs = %lld (0 = that sum)", c->n_envs_total,
                    (long long)c->env_id_base + c->n_envs);
    if (c->act_path == ANTSRL_ACT_CELL_META) {
        KP kp;
        fill_kp(c, &kp);
        if (!kp.meta)
            return fail(ANTSRL_E_UNSUPPORTED, "ANTSRL_ACT_CELL_META needs 2 pheromone channels, the generator's channel order "
                                              "([Ants, Phero0, Phero1, Anthill, Walls, Food(, Rocks)]), a perception of 128..368 values "
                                              "per ant over at most 64 cells, and at most 4096 ants per env");
    }
    return ANTSRL_OK;
}

// Scaled pheromone units (see ANTSRL_PHERO_AUTO in antsrl.h) apply to a centre-only filter whose
// coefficient is a genuine decay; anything else takes the explicit sweep.
static bool use_scaled(const AntsCfg *c)
{
    return c->phero_mode == ANTSRL_PHERO_AUTO && c->filter_radius == 0 && c->filter[0] > 0.5 &&
           c->filter[0] <= 1.0 && c->phero_threshold >= 0.0;
}

// Interleaved cell record {p0, p1, food, pad}: with scaled units there is no per-step sweep whose traffic the
// wider record would inflate, and a perception becomes ONE 16-byte gather per cell instead of an 8-byte
// and a 4-byte one (profiles/history/obs_write_probe.hip: 48-57 cycles per ant per CU against 70-77 on L2 hits,
// 180-197 against 275 from HBM).  Any other configuration keeps separate pheromone and food arrays.
static bool use_interleaved(const AntsCfg *c)
{
    return use_scaled(c) && c->n_phero == 2;
}

// Carves the workspace; with NULL bases only computes the sizes.  Two blocks (antsrl_create2): the cell records — what the
// kernels reach with scattered per-cell accesses — are taken from `rec_base` with a count of their own, everything else
// from `base`.  One block (antsrl_create: split == false, rec_base == base): one count, the records between the per-ant
// arrays and the bit maps.  bytes[0] / bytes[1]: the state / record block's size (one block: bytes[0] is all of it).
// `map` / `cap` / `count`: antsrl_workspace_map.
static void carve(const AntsCfg *c, DState *s, unsigned char *base, unsigned char *rec_base, bool split, size_t bytes[2],
                  AntsWsArray *map = nullptr, int32_t cap = 0, int32_t *count = nullptr)
{
    const size_t E = c->n_envs, N = c->n_ants, G = (size_t)c->w * c->h, Cn = c->n_phero, R = c->n_rocks;
    const size_t words = (G + 31) / 32;
    size_t off[2] = {0, 0};
    int32_t n_arrays = 0;
    auto take_from = [&](int block, const char *name, size_t nbytes) -> unsigned char * {
        unsigned char *b = block ? rec_base : base;
        size_t &o = off[split ? block : 0];
        unsigned char *ptr = b ? b + o : nullptr;
        if (map && n_arrays < cap) {
            AntsWsArray &a = map[n_arrays];
            memset(&a, 0, sizeof(a));
            strncpy(a.name, name, sizeof(a.name) - 1);
            a.block = split ? block : 0; a.offset = o; a.bytes = nbytes;
        }
        ++n_arrays;
        o = (o + nbytes + 255) / 256 * 256;
        return ptr;
    };
    auto take = [&](const char *name, size_t nbytes) { return take_from(0, name, nbytes); };
    auto take_rec = [&](const char *name, size_t nbytes) { return take_from(1, name, nbytes); };
    KP kp;
    fill_kp(c, &kp);
    DState d;
    d.x = (double *)take("x", 8 * E * N); d.y = (double *)take("y", 8 * E * N); d.theta = (double *)take("theta", 8 * E * N);
    d.prev_x = (double *)take("prev_x", 8 * E * N); d.prev_y = (double *)take("prev_y", 8 * E * N);
    d.prev_dist = (double *)take("prev_dist", 8 * E * N);
    d.holding = (float *)take("holding", 4 * E * N); d.seed = (float *)take("seed", 4 * E * N);
    d.prev_holding = (float *)take("prev_holding", 4 * E * N);
    d.activation = (float *)take("activation", 4 * E * N * Cn);
    d.mandibles = (uint8_t *)take("mandibles", E * N); d.reward_state = (uint8_t *)take("reward_state", E * N);
    d.dirty_cell = (int32_t *)take("dirty_cell", 4 * E * N);
    d.walldep_cell = (int32_t *)take("walldep_cell", 4 * E * N);
    if (use_interleaved(c)) { // one {p0, p1, food, pad} record per cell
        d.phero[0] = d.phero[1] = (float *)take_rec("records", 16 * E * G);
        d.food = d.phero[0] ? d.phero[0] + 2 : nullptr; // (inside the record array, whichever block holds it)
    } else {
        d.phero[0] = (float *)take_rec("phero0", 4 * E * G * Cn);
        d.phero[1] = use_scaled(c) ? d.phero[0] : (float *)take_rec("phero1", 4 * E * G * Cn); // no ping-pong when scaled
        d.food = (float *)take_rec("food", 4 * E * G * (size_t)kp.fs); // {food, META} records on the cell-meta path
    }
    d.walls_bits = (uint32_t *)take("walls_bits", 4 * E * words); d.area_bits = (uint32_t *)take("area_bits", 4 * E * words);
    d.explored_bits = (uint32_t *)take("explored_bits", 4 * E * words);
    d.big_pres = d.big_old = nullptr;
    if (!kp.meta && antsrl_act_needs_hbm_maps(kp)) {
        d.big_pres = (uint32_t *)take("big_pres", 4 * E * words);
        d.big_old = (uint32_t *)take("big_old", 4 * E * words);
    }
    d.primed_cur = kp.meta ? (uint8_t *)take("primed_cur", E) : nullptr;
    d.frames = kp.meta ? (AntFrame *)take("frames", sizeof(AntFrame) * E * N) : nullptr;
    d.anthill_xyr = (int32_t *)take("anthill_xyr", 4 * E * 3);
    d.anthill_food = (double *)take("anthill_food", 8 * E);
    d.rock_cx = (double *)take("rock_cx", 8 * E * (R ? R : 1)); d.rock_cy = (double *)take("rock_cy", 8 * E * (R ? R : 1));
    d.rock_r = (double *)take("rock_r", 8 * E * (R ? R : 1)); d.rock_w = (double *)take("rock_w", 8 * E * (R ? R : 1));
    d.timestep = (int32_t *)take("timestep", 4 * E);
    d.reward_primed = (uint8_t *)take("reward_primed", E);
    d.gen_discs = (int32_t *)take("gen_discs", 4 * E * ANTSRL_MAX_FOOD_DISCS * 3);
    d.gen_perlin = (int32_t *)take("gen_perlin", 4 * E * 2);
    d.pol_pack = (unsigned char *)take("pol_pack", ANTSRL_POL_PACK_BYTES);
    if (s) *s = d;
    if (count) *count = n_arrays;
    bytes[0] = off[0]; bytes[1] = off[1];
}

static void fill_kp(const AntsCfg *c, KP *p)
{
    memset(p, 0, sizeof(*p));
    p->E = c->n_envs; p->N = c->n_ants; p->W = c->w; p->H = c->h; p->C = c->n_phero; p->R = c->n_rocks;
    p->K = c->n_channels; p->r = c->perception_radius; p->P = 2 * p->r + 1; p->PP = p->P * p->P;
    p->words = (int)(((size_t)c->w * c->h + 31) / 32);
    int ht = 64;
    while (ht < 2 * c->n_ants) ht <<= 1;
    p->HT = ht;
    p->has_mask = c->has_mask; p->has_max_val = c->has_max_val; p->reward_kind = c->reward_kind;
    p->max_time = c->max_time; p->filter_radius = c->filter_radius;
    p->explore_on = c->reward_kind == ANTSRL_REWARD_EXPLORATION ||
                    (c->reward_kind == ANTSRL_REWARD_ALL &&
                     (c->fct_explore != 0.0 || c->fct_explore_holding != 0.0)); // reward_custom.py:87
    for (int k = 0; k < ANTSRL_MAX_CHANNELS; ++k) {
        p->ch_kind[k] = c->channel_kind[k];
        p->ch_arg[k] = c->channel_arg[k];
    }
    p->mand_first = p->mand_last = 0;
    for (int k = 0; k < c->n_channels; ++k) {
        const int op = c->channel_kind[k] == ANTSRL_CH_FOOD ? 1 : c->channel_kind[k] == ANTSRL_CH_ANTHILL ? 2 : 0;
        if (op && op != p->mand_last) {
            p->mand_first = p->mand_last;
            p->mand_last = op;
        }
    }
    memcpy(p->mask, c->mask, ANTSRL_MAX_PCELLS);
    p->delta = c->delta; p->fwd_delta = c->fwd_delta; p->max_speed = c->max_speed;
    p->max_rot_speed = c->max_rot_speed; p->carry = c->carry_speed_reduction;
    p->backward = c->backward_speed_reduction; p->max_hold = c->max_hold;
    p->max_val = c->phero_max_val; p->deposit_strength = c->deposit_strength;
    p->threshold = c->phero_threshold; p->reward_threshold = c->reward_threshold;
    p->fct_explore = c->fct_explore; p->fct_food = c->fct_food; p->fct_anthill = c->fct_anthill;
    p->fct_explore_holding = c->fct_explore_holding; p->fct_heading = c->fct_headinganthill;
    memcpy(p->filter, c->filter, sizeof(p->filter));
    {
        const int S = 2 * c->filter_radius + 1;
        for (int a = 0; a < S; ++a)
            for (int b = 0; b < S; ++b) {
                const double f = c->filter[a * S + b];
                const float hi = (float)f;
                p->ftap[(b * S + a) * 2 + 0] = hi;
                p->ftap[(b * S + a) * 2 + 1] = (float)(f - (double)hi);
            }
    }
    {
        // Rank-1 test: F == u v^T / F[i0][j0] around the largest tap, to 4 ulp of the largest tap.  Then the
        // stencil runs as a pass across the lanes followed by a pass along the march (2 x S taps instead of
        // S x S).  The taps u[a] * v[b] differ from F[a][b] by ~1e-16 relative: far inside the fp32 grid's
        // rounding, and unbiased like the hi + lo split of the full filter.
        const int S = 2 * c->filter_radius + 1;
        p->filter_sep = 0;
        if (S > 1) {
            int i0 = 0, j0 = 0;
            double big = 0.0;
            for (int a = 0; a < S; ++a)
                for (int b = 0; b < S; ++b)
                    if (fabs(c->filter[a * S + b]) > big) { big = fabs(c->filter[a * S + b]); i0 = a; j0 = b; }
            bool sep = big > 0.0;
            double u[2 * ANTSRL_MAX_FILTER_RADIUS + 1], v[2 * ANTSRL_MAX_FILTER_RADIUS + 1];
            for (int a = 0; a < S && sep; ++a) u[a] = c->filter[a * S + j0];
            for (int b = 0; b < S && sep; ++b) v[b] = c->filter[i0 * S + b] / c->filter[i0 * S + j0];
            for (int a = 0; a < S && sep; ++a)
                for (int b = 0; b < S; ++b)
                    if (fabs(u[a] * v[b] - c->filter[a * S + b]) > 1e-15 * big) sep = false;
            if (sep) {
                p->filter_sep = 1;
                for (int k = 0; k < S; ++k) {
                    const float uh = (float)u[k], vh = (float)v[k];
                    p->fsep_u[2 * k] = uh; p->fsep_u[2 * k + 1] = (float)(u[k] - (double)uh);
                    p->fsep_v[2 * k] = vh; p->fsep_v[2 * k + 1] = (float)(v[k] - (double)vh);
                }
            }
        }
    }
    p->rng_seed = c->rng_seed;
    p->env_id_base = (uint32_t)c->env_id_base;
    p->scaled = use_scaled(c) ? 1 : 0;
    p->ps = use_interleaved(c) ? 4 : c->n_phero;
    p->fs = use_interleaved(c) ? 4 : 1;
    p->g_now = p->g_dep = p->inv_g_dep = 1.0;
    // cell-meta path (k_move + k_perceive) for the reference's perception shapes (AntsCfg.act_path pins either).
    // (Round 2 first kept k_act for batches under 8192 ants — one launch fewer; with the deferred update the cell-meta
    // path is two launches per step as well and wins at every size: c1 13.8 against 15.3 us/step, 16 envs x 256 ants
    // 16.2 against 30.1 — profiles/r02/tiny_ab.txt.)
    p->meta = antsrl_meta_supported(*p) && c->act_path != ANTSRL_ACT_SINGLE_KERNEL ? 1 : 0;
    if (p->meta && p->fs == 1) p->fs = 2;
    // 2 x 4-cell blocks per line for the interleaved records (antsrl_device.h: KP::tiled)
    p->tiled = (p->meta && p->ps == 4 && p->fs == 4 && (c->w & 1) == 0 && (c->h & 3) == 0) ? 1 : 0;
    // 4 x 4-cell blocks per line for the 8-byte {food, META} records beside separate pheromone buffers (c4's layout: KP::ftile)
    p->ftile = (p->meta && p->fs == 2 && (c->w & 3) == 0 && (c->h & 3) == 0) ? 1 : 0;
}

// f0^S for the next observation, f0^(S+1) for the next deposit
static void set_decay(AntsHandle *h)
{
    if (!h->p.scaled) return;
    const double f0 = h->cfg.filter[0];
    h->p.g_now = pow(f0, (double)h->sweeps);
    h->p.g_dep = pow(f0, (double)(h->sweeps + 1));
    h->p.inv_g_dep = 1.0 / h->p.g_dep;
}

extern "C" int antsrl_workspace_bytes(const AntsCfg *cfg, size_t *bytes)
{
    int rc = validate(cfg);
    if (rc) return rc;
    if (!bytes) return fail(ANTSRL_E_INVALID, "bytes is NULL");
    size_t b[2];
    carve(cfg, nullptr, nullptr, nullptr, false, b);
    *bytes = b[0];
    return ANTSRL_OK;
}

extern "C" int antsrl_workspace_bytes2(const AntsCfg *cfg, size_t *state_bytes, size_t *record_bytes)
{
    int rc = validate(cfg);
    if (rc) return rc;
    size_t b[2];
    carve(cfg, nullptr, nullptr, nullptr, true, b);
    if (state_bytes) *state_bytes = b[0];
    if (record_bytes) *record_bytes = b[1];
    return ANTSRL_OK;
}

extern "C" int antsrl_workspace_map(const AntsCfg *cfg, int split, AntsWsArray *entries, int32_t cap, int32_t *count)
{
    int rc = validate(cfg);
    if (rc) return rc;
    if (!count) return fail(ANTSRL_E_INVALID, "count is NULL");
    if (cap < 0 || (cap > 0 && !entries)) return fail(ANTSRL_E_INVALID, "entries is NULL or cap < 0");
    size_t b[2];
    carve(cfg, nullptr, nullptr, nullptr, split != 0, b, entries, cap, count);
    return ANTSRL_OK;
}

// The checkpoint's device block (include/antsrl.h, "CHECKPOINT"): every array of the carve but pol_pack, in carve order,
// each stored whole and rounded up to 256 bytes — the carve's own sequence with the two blocks' counts merged into one, so
// it does not depend on `split`.  Fills `ws` (the arrays where they lie in a workspace carved with `split` over `base` /
// `rec_base`; may be NULL with NULL bases) and `ck` side by side, ENV_COPY_MAX_ARRAYS entries each; returns their number.
static int32_t ckpt_arrays(const AntsCfg *c, bool split, unsigned char *base, unsigned char *rec_base, unsigned char **ptrs,
                           AntsCkptArray *ck, size_t *device_bytes)
{
    AntsWsArray all[ENV_COPY_MAX_ARRAYS + 1];
    int32_t count = 0, n = 0;
    size_t b[2], off = 0;
    carve(c, nullptr, nullptr, nullptr, split, b, all, ENV_COPY_MAX_ARRAYS + 1, &count);
    if (count > ENV_COPY_MAX_ARRAYS + 1) return -1;
    for (int32_t i = 0; i < count; ++i) {
        if (strcmp(all[i].name, "pol_pack") == 0) continue; // the caller's policy, not state: the agent installs it again
        if (ptrs) ptrs[n] = (all[i].block ? rec_base : base) + all[i].offset;
        memset(&ck[n], 0, sizeof(ck[n]));
        memcpy(ck[n].name, all[i].name, sizeof(ck[n].name));
        ck[n].offset = off;
        ck[n].bytes_per_env = all[i].bytes / (uint64_t)c->n_envs; // (every array of the carve is environment-major)
        off = (off + all[i].bytes + 255) / 256 * 256;
        ++n;
    }
    *device_bytes = off;
    return n;
}

extern "C" int antsrl_checkpoint_map(const AntsCfg *cfg, AntsCkptArray *entries, int32_t cap, int32_t *count,
                                     size_t *device_bytes, size_t *host_bytes)
{
    int rc = validate(cfg);
    if (rc) return rc;
    if (cap < 0 || (cap > 0 && !entries)) return fail(ANTSRL_E_INVALID, "checkpoint_map: entries is NULL or cap < 0");
    AntsCkptArray ck[ENV_COPY_MAX_ARRAYS];
    size_t dev = 0;
    const int32_t n = ckpt_arrays(cfg, false, nullptr, nullptr, nullptr, ck, &dev);
    if (n < 0) return fail(ANTSRL_E_UNSUPPORTED, "checkpoint_map: more than %d arrays in the carve", ENV_COPY_MAX_ARRAYS);
    for (int32_t i = 0; i < n && i < cap; ++i) entries[i] = ck[i];
    if (count) *count = n;
    if (device_bytes) *device_bytes = dev;
    if (host_bytes) *host_bytes = sizeof(AntsCkptBlob);
    return ANTSRL_OK;
}

// the handle over a carved workspace: one block (split == false, record_ws == workspace) or two
static int create_handle(const AntsCfg *cfg, void *state_ws, void *record_ws, bool split, const size_t need[2], AntsHandle **out)
{
    AntsHandle *h = new (std::nothrow) AntsHandle();
    if (!h) return fail(ANTSRL_E_NOMEM, "out of host memory");
    h->cfg = *cfg;
    fill_kp(cfg, &h->p);
    size_t b[2];
    carve(cfg, &h->p.s, (unsigned char *)state_ws, (unsigned char *)record_ws, split, b);
    h->ws_bytes[0] = need[0]; h->ws_bytes[1] = need[1];
    if (!h->p.meta && !antsrl_act_fits(h->p)) {
        delete h;
        return fail(ANTSRL_E_UNSUPPORTED,
                    "%d ants with a %dx%d perception need more than 160 KiB of LDS per workgroup "
                    "(per-ant frames, the collision hash and the row staging are kept in LDS)", cfg->n_ants,
                    2 * cfg->perception_radius + 1, 2 * cfg->perception_radius + 1);
    }
    *out = h;
    return ANTSRL_OK;
}

extern "C" int antsrl_create(const AntsCfg *cfg, void *workspace, size_t workspace_bytes, AntsHandle **out)
{
    int rc = validate(cfg);
    if (rc) return rc;
    if (!out) return fail(ANTSRL_E_INVALID, "out is NULL");
    if (!workspace) return fail(ANTSRL_E_INVALID, "workspace is NULL");
    if (((uintptr_t)workspace & 255) != 0) return fail(ANTSRL_E_INVALID, "workspace must be 256-byte aligned");
    size_t need[2];
    carve(cfg, nullptr, nullptr, nullptr, false, need);
    if (workspace_bytes < need[0])
        return fail(ANTSRL_E_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need[0]);
    return create_handle(cfg, workspace, workspace, false, need, out);
}

extern "C" int antsrl_create2(const AntsCfg *cfg, void *state_ws, size_t state_bytes, void *record_ws, size_t record_bytes,
                              AntsHandle **out)
{
    int rc = validate(cfg);
    if (rc) return rc;
    if (!out) return fail(ANTSRL_E_INVALID, "out is NULL");
    if (!state_ws || !record_ws) return fail(ANTSRL_E_INVALID, "state_ws or record_ws is NULL");
    if ((((uintptr_t)state_ws | (uintptr_t)record_ws) & 255) != 0)
        return fail(ANTSRL_E_INVALID, "state_ws and record_ws must be 256-byte aligned");
    size_t need[2];
    carve(cfg, nullptr, nullptr, nullptr, true, need);
    if (state_bytes < need[0])
        return fail(ANTSRL_E_NOMEM, "state block too small: %zu < %zu bytes", state_bytes, need[0]);
    if (record_bytes < need[1])
        return fail(ANTSRL_E_NOMEM, "record block too small: %zu < %zu bytes", record_bytes, need[1]);
    const uintptr_t s0 = (uintptr_t)state_ws, r0 = (uintptr_t)record_ws;
    if (s0 < r0 + need[1] && r0 < s0 + need[0])
        return fail(ANTSRL_E_INVALID, "the state block and the record block overlap");
    return create_handle(cfg, state_ws, record_ws, true, need, out);
}

extern "C" void antsrl_destroy(AntsHandle *h) { delete h; }

// The start of an episode, once the launch that writes its state has succeeded (ahead of it the caller has dropped
// `pend_update` and `phase_next` of the state being replaced).
static void begin_episode(AntsHandle *h, bool need_wall_clear, uint64_t episode_seed)
{
    h->p.deposit_strength = h->cfg.deposit_strength;
    h->cur = 0; h->steps_since_update = 0; h->need_full_collect = true; h->is_reset = true; h->episode_over = false;
    h->sweeps = 0; h->need_wall_clear = need_wall_clear; h->host_timestep = 1;
    h->obs_seq = 0; h->sum_obs = 0; h->sum_due = false; h->sum_live = false;
    h->episode_seed = episode_seed;
    set_decay(h);
}

extern "C" int antsrl_reset(AntsHandle *h, const AntsInit *init, void *stream)
{
    if (!h || !init) return fail(ANTSRL_E_INVALID, "NULL handle or init");
    if (!init->ants_xyt || !init->seed || !init->walls || !init->food || !init->anthill_xyr)
        return fail(ANTSRL_E_INVALID, "AntsInit: ants_xyt, seed, walls, food, anthill_xyr are required");
    if (h->p.R > 0 && !init->rocks) return fail(ANTSRL_E_INVALID, "AntsInit.rocks is NULL but n_rocks > 0");
    h->pend_update = false; // (a deferred update of the state being replaced)
    h->phase_next = 0;
    if (int rc = enqueued(antsrl_launch_reset(h->p, init, (hipStream_t)stream), "reset")) return rc;
    begin_episode(h, h->p.scaled && init->phero != nullptr, h->episode_seed); // (the seed is the generator's: it stays)
    return ANTSRL_OK;
}

// np.random.seed(seed * 5) takes 32 bits (environment_generator.py:55): env e draws from seed + env_id_base + e.  Checked at
// every (auto-)reset: numpy raises past 2^32, a wrapped seed would silently replay an earlier episode.  (Written so that
// no intermediate can wrap in uint64.)
static int check_gen_seed(const AntsHandle *h, const AntsGen &g, uint64_t seed)
{
    const uint64_t top = (uint64_t)h->p.env_id_base + (uint64_t)h->p.E; // < 2^31
    const uint64_t lim = 0xFFFFFFFFull / 5u;                            // (top may exceed it: compare before subtracting)
    if (g.rng_kind == ANTSRL_RNG_REFERENCE && (top > lim || seed > lim - top))
        return fail(ANTSRL_E_INVALID, "ANTSRL_RNG_REFERENCE: (episode_seed + env_id_base + n_envs) * 5 must stay below 2^32 (np.random.seed)");
    return ANTSRL_OK;
}

static int do_generate(AntsHandle *h, uint64_t seed, hipStream_t st)
{
    int rc = check_gen_seed(h, h->gen, seed);
    if (rc) return rc;
    h->pend_update = false; // (a deferred update of the state being replaced)
    h->phase_next = 0;
    if (int rc = enqueued(antsrl_launch_generate(h->p, h->gen, seed, st), "generate")) return rc;
    begin_episode(h, false, seed);
    return ANTSRL_OK;
}

extern "C" int antsrl_generate(AntsHandle *h, const AntsGen *gen, uint64_t episode_seed, void *stream)
{
    if (!h || !gen) return fail(ANTSRL_E_INVALID, "NULL handle or gen");
    if (gen->n_food_discs < 0 || gen->n_food_discs > ANTSRL_MAX_FOOD_DISCS)
        return fail(ANTSRL_E_INVALID, "n_food_discs must be in 0..%d", ANTSRL_MAX_FOOD_DISCS);
    if (gen->food_rmin < 0 || gen->food_rmax < gen->food_rmin) return fail(ANTSRL_E_INVALID, "bad food radii");
    if (gen->wall_kind == ANTSRL_WALLS_BERNOULLI) {
        if (!(gen->wall_density >= 0.0 && gen->wall_density <= 1.0)) return fail(ANTSRL_E_INVALID, "bad wall_density");
    } else if (gen->wall_kind == ANTSRL_WALLS_PERLIN) {
        if (!(gen->wall_density >= -1.0 && gen->wall_density <= 1.0) || gen->perlin_octaves < 1 || gen->perlin_octaves > 8 ||
            !(gen->perlin_scale > 0.0) || !(gen->perlin_persistence > 0.0) || !(gen->perlin_lacunarity > 0.0))
            return fail(ANTSRL_E_INVALID, "bad Perlin wall parameters (density in [-1, 1], 1..8 octaves, positive "
                                          "scale / persistence / lacunarity)");
    } else if (gen->wall_kind == ANTSRL_WALLS_INPUT) {
        if (!gen->walls_input) return fail(ANTSRL_E_INVALID, "ANTSRL_WALLS_INPUT needs AntsGen.walls_input");
    } else {
        return fail(ANTSRL_E_INVALID, "bad wall_kind %d", gen->wall_kind);
    }
    if (gen->rng_kind != ANTSRL_RNG_COUNTER && gen->rng_kind != ANTSRL_RNG_REFERENCE)
        return fail(ANTSRL_E_INVALID, "bad rng_kind %d", gen->rng_kind);
    if (gen->rng_kind == ANTSRL_RNG_REFERENCE) {
        if (gen->wall_kind == ANTSRL_WALLS_BERNOULLI && gen->wall_density != 0.0)
            return fail(ANTSRL_E_UNSUPPORTED, "the reference has no Bernoulli walls generator: with ANTSRL_RNG_REFERENCE use "
                                              "ANTSRL_WALLS_PERLIN, ANTSRL_WALLS_INPUT or wall_density 0");
        // (the 32-bit limit of np.random.seed(seed * 5) is checked in do_generate, for this and every auto-reset episode)
    }
    int rc = check_gen_seed(h, *gen, episode_seed); // (before anything of the handle changes: a refused call leaves it as it was)
    if (rc) return rc;
    h->gen = *gen;
    h->has_gen = true;
    return do_generate(h, episode_seed, (hipStream_t)stream);
}

// (only k_act can refuse the format: the cell-meta path takes bfloat16 observations at any grid size)
static int bf16_unsupported()
{
    return fail(ANTSRL_E_UNSUPPORTED, "bfloat16 observations on the single-kernel path (k_act) need 2 pheromone channels, the "
                                      "generator's channel order ([Ants, Phero0, Phero1, Anthill, Walls, Food(, Rocks)]), a perception of "
                                      "at most 64 cells and a grid whose bit maps fit LDS (up to ~600k cells); the cell-meta path "
                                      "(ANTSRL_Q_CELL_META) has no grid limit");
}

extern "C" int antsrl_set_obs_format(AntsHandle *h, int format)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (format != ANTSRL_OBS_F32 && format != ANTSRL_OBS_BF16) return fail(ANTSRL_E_INVALID, "bad observation format %d", format);
    if ((format == ANTSRL_OBS_BF16) != h->obs_bf16) h->obs_pitch = 0; // (a row stride is a whole number of lines of ONE element size)
    h->obs_bf16 = format == ANTSRL_OBS_BF16;
    if (!h->obs_bf16) h->pol = PolArgs{}; // (the in-loop policy reads bfloat16 rows)
    return ANTSRL_OK;
}

extern "C" int antsrl_set_obs_row_stride(AntsHandle *h, int32_t stride_elems)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    const int32_t row = h->p.PP * h->p.K, esz = h->obs_bf16 ? 2 : 4;
    if (stride_elems == 0 || stride_elems == row) {
        h->obs_pitch = 0;
        return ANTSRL_OK;
    }
    if (stride_elems < row || ((long long)stride_elems * esz) % 128 != 0 || stride_elems > row + 128 / esz)
        return fail(ANTSRL_E_INVALID, "obs row stride %d: 0 (dense) or the row's %d elements rounded up to whole 128-byte lines (%d)",
                    stride_elems, row, (row * esz + 127) / 128 * 128 / esz);
    if (!h->p.meta) return fail(ANTSRL_E_UNSUPPORTED, "antsrl_set_obs_row_stride needs the cell-meta path (ANTSRL_Q_CELL_META)");
    if (h->pol.pack) // (refused HERE, not in the middle of a step whose move has already been enqueued)
        return fail(ANTSRL_E_UNSUPPORTED, "a padded observation row stride and the in-loop policy exclude each other (the net reads a "
                                          "dense tile image): switch the policy off first (antsrl_set_inloop_policy with w1 == NULL)");
    h->obs_pitch = (uint32_t)stride_elems;
    return ANTSRL_OK;
}

extern "C" int antsrl_set_perceive_path(AntsHandle *h, int path)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (path != ANTSRL_PERCEIVE_AUTO && path != ANTSRL_PERCEIVE_GENERIC && path != ANTSRL_PERCEIVE_FAST_NOSKIP)
        return fail(ANTSRL_E_INVALID, "bad perceive path %d", path);
    h->prc_generic = path == ANTSRL_PERCEIVE_GENERIC;
    h->prc_noskip = path == ANTSRL_PERCEIVE_FAST_NOSKIP;
    return ANTSRL_OK;
}

// The explored summary (antsrl_explored.h) is kept and consumed by this handle as it is set up now.  (Bits set while it
// was stay true whatever the path is switched to in between: they are only ever cleared by a reset.)
static bool summary_on(const AntsHandle *h)
{
    return !h->prc_generic && !h->prc_noskip && antsrl_explored_summary_supported(h->p, h->pol.pack != nullptr && h->obs_bf16);
}
// The refresh cadence, in observations since the last reset: behind observation 256, 512 and 1024, then behind every
// 1024th.  Until an episode's first refresh k_perceive is not told of the summary at all (sum_live): no bit can be set, the
// launch is spared the summary's loads.  (From 128 on, the first 400 steps of a c3 episode still ran 0.5 % slower than the
// parent's, the parent's spread being 0.4 %: early in an episode the ants stand close together, their patches share lines
// anyway, and the skip buys less than its prologue costs.)  One refresh reads the tiles still open — a line each, whole where the sample is explored: 0.09 ms at c3 behind
// observation 63, 0.06 ms behind 399 — and early in an episode the frontier's tiles are read again at every one.  Behind every
// 64th observation from 64 on the first 400 steps of a c3 episode ran 1.9 % SLOWER than the parent's; exploration slows
// down as it completes (0.87 of the map at age 200, 0.97 at 300, 0.999 at 600), so the intervals may double
// (profiles/r08/ROUND_NOTES.md).
#define SUMMARY_FIRST 256u
#define SUMMARY_STEADY 1024u
static bool summary_cadence(uint32_t n)
{
    return n >= SUMMARY_FIRST && (n <= SUMMARY_STEADY ? (n & (n - 1u)) == 0u : n % SUMMARY_STEADY == 0u);
}

int flush_pending(AntsHandle *h, hipStream_t st) // antsrl_handle.h
{
    if (!h->pend_update) return ANTSRL_OK;
    h->pend_update = false;
    return enqueued(antsrl_launch_update(h->pend_p, nullptr, h->pend_out_buf, st), "deferred update");
}

int handle_ready(const AntsHandle *h, MidUpdate mid) // antsrl_handle.h
{
    if (!h->is_reset && h->episode_over)
        return fail(ANTSRL_E_INVALID, "the episode is over and its auto-reset was refused (episode seed past np.random.seed's 32 bits): "
                                      "call antsrl_reset or antsrl_generate");
    if (!h->is_reset) return fail(ANTSRL_E_INVALID, "antsrl_reset has not been called on this handle");
    if (h->phase_next && mid == MID_UPDATE_REFUSED)
        return fail(ANTSRL_E_INVALID, "an Environment.update is in progress (antsrl_update_phase %d of 4 is next): finish it first", h->phase_next);
    return ANTSRL_OK;
}

// One observation on the cell-meta path: k_move (with the action phases when `stepping`) then k_perceive.
static int meta_observe(AntsHandle *h, const int8_t *rot, const int8_t *ph, float *obs, float *agent_state,
                        float *reward, uint8_t *done, bool stepping, hipStream_t st, bool timed)
{
    if (obs && h->obs_pitch != 0 && h->obs_pitch != (uint32_t)(h->p.PP * h->p.K) && h->pol.pack && h->obs_bf16) // (both setters refuse the
        return fail(ANTSRL_E_UNSUPPORTED, "a padded observation row stride and the in-loop policy exclude each other"); // pair; before any launch)
    if (h->obs_seq >= META_NEVER - 2) { // explored stamps: re-base long before the counter can reach "never"
        if (int rc = enqueued(antsrl_launch_meta_rebase(h->p, st), "explored-stamp rebase")) return rc;
        h->obs_seq = 0;
    }
    h->obs_seq++;
    bool frames = false; // k_update_move leaves the ants' perception frames for the k_perceive right behind it
    if (h->pend_update && stepping) { // the previous step's update and this step's move in one launch
        h->pend_update = false;
        // Frames from k_update_move pay where k_perceive is latency-bound — the in-loop policy's launches, whose rows are
        // bfloat16 or stay in LDS: c5 -2.5 %, k_perceive -5 % — and cost 1-2 us of a second sincos where it is bound by its
        // float32 store stream, which hides the prologue anyway (c3 / c2 / c4: +1 %; profiles/r04/frames_ab.txt).
        frames = h->pol.pack != nullptr;
        if (int rc = enqueued(antsrl_launch_update_move(h->p, h->pend_out_buf, h->pend_p.g_dep, h->pend_p.inv_g_dep, rot, ph, done,
                                                        h->obs_seq, st, frames),
                              "update + move"))
            return rc;
    } else {
        if (int rc = flush_pending(h, st)) return rc;
        if (int rc = enqueued(antsrl_launch_move(h->p, rot, ph, done, stepping ? 1 : 0, h->obs_seq, st), "move")) return rc;
    }
    if (timed) (void)hipEventRecord(h->ev[2], st);
    hipError_t e = antsrl_launch_perceive(h->p, h->cur, obs, agent_state, reward,
                                          (stepping ? ACT_STEP : 0) | (obs ? ACT_HAS_OBS : 0) | (frames ? ACT_FRAMES : 0) |
                                              ((obs || h->pol.pack) && h->obs_bf16 ? ACT_OBS_BF16 : 0) | // (act-only: rows in LDS, bf16)
                                              (h->sum_live && summary_on(h) ? ACT_SUMMARY : 0),
                                          h->obs_seq, st, &h->pol, h->obs_pitch, h->prc_generic);
    if (e == hipErrorNotSupported)
        return fail(ANTSRL_E_UNSUPPORTED, "a padded observation row stride and the in-loop policy exclude each other (the net reads a dense tile image)");
    if (int rc = enqueued(e, "perceive")) return rc;
    if (summary_cadence(++h->sum_obs) && summary_on(h)) h->sum_due = true; // (enqueued by the caller: summary_refresh_due)
    return ANTSRL_OK;
}

// One observation on the single-kernel path (k_act), meta_observe's counterpart; `what`: the caller's word for hip_fail.
static int act_observe(AntsHandle *h, const int8_t *rot, const int8_t *ph, float *obs, float *agent_state, float *reward,
                       uint8_t *done, bool stepping, hipStream_t st, bool timed, const char *what)
{
    if (obs && h->obs_pitch) return fail(ANTSRL_E_UNSUPPORTED, "antsrl_set_obs_row_stride needs the cell-meta path (ANTSRL_Q_CELL_META)");
    if (timed) (void)hipEventRecord(h->ev[2], st);
    hipError_t e = antsrl_launch_act(h->p, rot, ph, h->cur, obs, agent_state, reward, done,
                                     (stepping ? ACT_STEP : 0) | (obs ? ACT_HAS_OBS : 0) | (obs && h->obs_bf16 ? ACT_OBS_BF16 : 0), st);
    if (e == hipErrorNotSupported) return bf16_unsupported();
    return enqueued(e, what);
}

// The summary's refresh when the cadence asks for one: BEHIND the observation whose marks it may count (bits are set
// between observations only), and — in antsrl_step_update — behind the timing event that closes k_perceive's bracket: its
// time is the step's, not the k_update_move bracket's or the k_perceive bracket's.
static int summary_refresh_due(AntsHandle *h, hipStream_t st)
{
    if (!h->sum_due) return ANTSRL_OK;
    h->sum_due = false;
    h->sum_live = true;
    return enqueued(antsrl_launch_explored_summary(h->p, st), "explored summary");
}

static int do_step(AntsHandle *h, const int8_t *rot, const int8_t *ph, float *obs, float *agent_state,
                   float *reward, uint8_t *done, hipStream_t st, bool timed = false)
{
    if (ph && h->p.C != 2) // Ants.activate_pheromone hard-codes two channels, ants.py:89-96
        return fail(ANTSRL_E_INVALID, "pheromone actions need exactly 2 pheromone channels (ants.py:89-96)");
    if (h->steps_since_update > 0) h->need_full_collect = true; // dirty-cell list would be overwritten
    int rc = h->p.meta ? meta_observe(h, rot, ph, obs, agent_state, reward, done, true, st, timed)
                       : act_observe(h, rot, ph, obs, agent_state, reward, done, true, st, timed, "step");
    if (rc) return rc;
    h->steps_since_update++;
    return ANTSRL_OK;
}

// The two ends of an Environment.update that antsrl_update and antsrl_update_phase share (they must stay bit-identical).
// Scaled units, ahead of the update's first kernel: re-base the units long before u = v / f0^S can overflow fp32
// (value-preserving), then the Walls pass of this update (walls.py:30) on the initial grid, before its deposits land.
static int update_prepare_scaled(AntsHandle *h, hipStream_t st)
{
    if (h->p.g_dep < 1e-20) {
        if (int rc = enqueued(antsrl_launch_phero_renorm(h->p, st), "pheromone renorm")) return rc;
        h->sweeps = 0;
        set_decay(h);
    }
    if (h->need_wall_clear) {
        if (int rc = enqueued(antsrl_launch_phero_wall_clear(h->p, st), "pheromone wall clear")) return rc;
        h->need_wall_clear = false;
    }
    return ANTSRL_OK;
}

// Behind the update's last kernel: Anthill.update over the whole grid when due, then the environment's timestep advances.
// `flip`: the swept grid becomes the current one here (antsrl_update_phase has flipped in its ROCKS_PHEROMONE phase).
static int update_close(AntsHandle *h, hipStream_t st, bool flip)
{
    if (h->need_full_collect) {
        if (int rc = enqueued(antsrl_launch_collect_full(h->p, st), "anthill collect")) return rc;
        h->need_full_collect = false;
    }
    if (flip) h->cur ^= 1;
    h->steps_since_update = 0;
    h->host_timestep++;
    return ANTSRL_OK;
}

static int do_update(AntsHandle *h, const double *jitter, hipStream_t st, bool sweep_done, bool may_defer)
{
    if (int rc = flush_pending(h, st)) return rc; // (two updates in a row)
    if (h->p.scaled) {
        if (int rc = update_prepare_scaled(h, st)) return rc;
    } else if (!sweep_done) {
        if (int rc = enqueued(antsrl_launch_sweep(h->p, h->cur, st), "pheromone sweep")) return rc;
    }
    // Deferred: with the library's own wall jitter (no caller buffer to outlive the call) and nothing that has to
    // run after the update kernel in this call, the kernel is left for the next step's k_update_move.
    if (may_defer && !jitter && !h->need_full_collect && antsrl_update_move_supported(h->p)) {
        h->pend_update = true;
        h->pend_p = h->p;
        h->pend_out_buf = h->p.scaled ? 0 : h->cur ^ 1;
    } else {
        if (int rc = enqueued(antsrl_launch_update(h->p, jitter, h->p.scaled ? 0 : h->cur ^ 1, st), "update")) return rc;
    }
    if (h->p.scaled) {
        h->sweeps++;
        set_decay(h);
    }
    return update_close(h, st, !h->p.scaled);
}

extern "C" int antsrl_step(AntsHandle *h, const int8_t *rotation, const int8_t *phero, float *obs,
                           float *agent_state, float *reward, uint8_t *done, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if (!agent_state || !reward || !done) return fail(ANTSRL_E_INVALID, "agent_state, reward, done are required");
    int rc = do_step(h, rotation, phero, obs, agent_state, reward, done, (hipStream_t)stream);
    return rc ? rc : summary_refresh_due(h, (hipStream_t)stream);
}

extern "C" int antsrl_observe(AntsHandle *h, float *obs, float *agent_state, float *reward, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if (!h->p.meta)
        return act_observe(h, nullptr, nullptr, obs, agent_state, reward, nullptr, false, (hipStream_t)stream, false, "observe");
    int rc = meta_observe(h, nullptr, nullptr, obs, agent_state, reward, nullptr, false, (hipStream_t)stream, false);
    return rc ? rc : summary_refresh_due(h, (hipStream_t)stream);
}

extern "C" int antsrl_update(AntsHandle *h, const double *wall_jitter, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    return do_update(h, wall_jitter, (hipStream_t)stream, false, true);
}

// Environment.update one reference step at a time (include/antsrl.h).  Bit-identical to antsrl_update: the same device
// functions in the same order, cut at the launch boundaries.
extern "C" int antsrl_update_phase(AntsHandle *h, int phase, const double *wall_jitter, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (int rc = handle_ready(h, MID_UPDATE_ALLOWED)) return rc; // (the phase in progress is checked below)
    if (phase < ANTSRL_PHASE_WALLS || phase > ANTSRL_PHASE_ANTHILL) return fail(ANTSRL_E_INVALID, "bad phase %d", phase);
    if (phase != h->phase_next)
        return fail(ANTSRL_E_INVALID, "antsrl_update_phase: phase %d is next, got %d (WALLS, ROCKS_PHEROMONE, ANTS, ANTHILL in order)", h->phase_next, phase);
    hipStream_t st = (hipStream_t)stream;
    const int out_buf = h->p.scaled ? 0 : h->cur; // (as it stands when the phase's update kernel is enqueued)
    if (phase == ANTSRL_PHASE_WALLS) { // walls.py:22-30 (update_step -1)
        if (int rc = flush_pending(h, st)) return rc;
        if (h->p.scaled) {
            if (int rc = update_prepare_scaled(h, st)) return rc;
        } else { // `phero[map] = 0` as a step of its own (the sweep of the next phase does it again, to the same effect)
            if (int rc = enqueued(antsrl_launch_phero_wall_clear(h->p, st, h->cur), "pheromone wall clear")) return rc;
        }
        if (int rc = enqueued(antsrl_launch_update(h->p, wall_jitter, out_buf, st, UPD_WALLS), "update: walls")) return rc;
    } else if (phase == ANTSRL_PHASE_ROCKS_PHEROMONE) { // circle_obstacles.py:32-58, pheromone.py:43-45 (update_step 0)
        if (int rc = enqueued(antsrl_launch_update(h->p, nullptr, out_buf, st, UPD_ROCKS), "update: rocks")) return rc;
        if (h->p.scaled) { // the conceptual sweep: readers materialise one more decay from here on; the deposit of the
            h->sweeps++;   // ANTS phase lands "after the sweep of this update" = at the new g_now
            set_decay(h);
        } else {
            if (int rc = enqueued(antsrl_launch_sweep(h->p, h->cur, st), "pheromone sweep")) return rc;
            h->cur ^= 1; // readers (and the deposit) see the swept grid from here on
        }
    } else if (phase == ANTSRL_PHASE_ANTS) { // ants.py:123-130 (update_step 999)
        KP kp = h->p;
        if (kp.scaled) { // (the units were advanced in the previous phase: the deposit factor is the CURRENT decay)
            kp.g_dep = kp.g_now;
            kp.inv_g_dep = 1.0 / kp.g_dep;
        }
        if (int rc = enqueued(antsrl_launch_update(kp, nullptr, out_buf, st, UPD_ANTS), "update: ants")) return rc;
    } else { // anthill.py:41-46 (update_step 1000); the environment's timestep advances here
        if (int rc = enqueued(antsrl_launch_update(h->p, nullptr, out_buf, st, UPD_ANTHILL), "update: anthill")) return rc;
        if (int rc = update_close(h, st, false)) return rc;
    }
    h->phase_next = (phase + 1) % 4;
    return ANTSRL_OK;
}

extern "C" int antsrl_refresh_explored_summary(AntsHandle *h, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if (!summary_on(h)) return ANTSRL_OK;
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc; // (as antsrl_read_state: behind a deferred update)
    h->sum_live = true;
    return enqueued(antsrl_launch_explored_summary(h->p, (hipStream_t)stream), "explored summary");
}

extern "C" int antsrl_flush(AntsHandle *h, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    return flush_pending(h, (hipStream_t)stream);
}

// ---- checkpoint, restore, fork (include/antsrl.h, "CHECKPOINT") ---------------------------------------------------------
// The arrays of this handle's workspace beside their places in a checkpoint block, as k_env_copy's table; `blk` NULL: the
// fork's table (rows inside the workspace, bytes per environment).  The workspace's bases are the first array of each block.
static int ckpt_table(const AntsHandle *h, EnvCopyTable *t, unsigned char *blk, bool to_block, const char *who)
{
    const bool split = h->ws_bytes[1] != 0;
    unsigned char *base = (unsigned char *)h->p.s.x, *rec_base = split ? (unsigned char *)h->p.s.phero[0] : base;
    unsigned char *ptrs[ENV_COPY_MAX_ARRAYS];
    AntsCkptArray ck[ENV_COPY_MAX_ARRAYS];
    size_t dev = 0;
    const int32_t n = ckpt_arrays(&h->cfg, split, base, rec_base, ptrs, ck, &dev);
    if (n < 0) return fail(ANTSRL_E_UNSUPPORTED, "%s: more than %d arrays in the carve", who, ENV_COPY_MAX_ARRAYS);
    if (blk) { // (both directions write one range and read the other: neither may reach into the workspace)
        const uintptr_t b0 = (uintptr_t)blk, s0 = (uintptr_t)base, r0 = (uintptr_t)rec_base;
        if ((b0 < s0 + h->ws_bytes[0] && s0 < b0 + dev) || (split && b0 < r0 + h->ws_bytes[1] && r0 < b0 + dev))
            return fail(ANTSRL_E_INVALID, "%s: device_block overlaps the handle's workspace", who);
    }
    memset(t, 0, sizeof(*t));
    uint64_t chunks = 0;
    for (int32_t i = 0; i < n; ++i) {
        EnvCopyArray &a = t->a[i];
        a.bytes = blk ? ck[i].bytes_per_env * (uint64_t)h->p.E : ck[i].bytes_per_env;
        unsigned char *in_blk = blk ? blk + ck[i].offset : ptrs[i];
        a.src = to_block ? ptrs[i] : in_blk;
        a.dst = to_block ? in_blk : ptrs[i];
        a.first_chunk = (uint32_t)chunks;
        chunks += env_copy_chunks(a.bytes);
    }
    if (chunks > 0x7fffffffull) return fail(ANTSRL_E_UNSUPPORTED, "%s: the workspace is too large for one copy", who);
    t->n_arrays = n;
    t->chunks_per_row = (uint32_t)chunks;
    return ANTSRL_OK;
}

// the name of the AntsCfg field that holds byte `off`
static const char *cfg_field_at(size_t off)
{
#define CFG_FIELD(f) \
    if (off >= offsetof(AntsCfg, f) && off < offsetof(AntsCfg, f) + sizeof(((AntsCfg *)0)->f)) return #f;
    CFG_FIELD(abi_version) CFG_FIELD(n_envs) CFG_FIELD(n_ants) CFG_FIELD(w) CFG_FIELD(h) CFG_FIELD(n_phero) CFG_FIELD(n_rocks)
    CFG_FIELD(max_time) CFG_FIELD(perception_radius) CFG_FIELD(n_channels) CFG_FIELD(channel_kind) CFG_FIELD(channel_arg)
    CFG_FIELD(has_mask) CFG_FIELD(mask) CFG_FIELD(delta) CFG_FIELD(fwd_delta) CFG_FIELD(max_speed) CFG_FIELD(max_rot_speed)
    CFG_FIELD(carry_speed_reduction) CFG_FIELD(backward_speed_reduction) CFG_FIELD(max_hold) CFG_FIELD(has_max_val)
    CFG_FIELD(filter_radius) CFG_FIELD(phero_max_val) CFG_FIELD(deposit_strength) CFG_FIELD(phero_threshold) CFG_FIELD(filter)
    CFG_FIELD(reward_kind) CFG_FIELD(phero_mode) CFG_FIELD(reward_threshold) CFG_FIELD(fct_explore) CFG_FIELD(fct_food)
    CFG_FIELD(fct_anthill) CFG_FIELD(fct_explore_holding) CFG_FIELD(fct_headinganthill) CFG_FIELD(rng_seed) CFG_FIELD(act_path)
    CFG_FIELD(env_id_base) CFG_FIELD(n_envs_total)
#undef CFG_FIELD
    return "padding";
}

extern "C" int antsrl_checkpoint_save(AntsHandle *h, void *device_block, void *host_blob, void *stream)
{
    if (!h || !device_block || !host_blob) return fail(ANTSRL_E_INVALID, "checkpoint_save: NULL handle, device_block or host_blob");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if ((uintptr_t)device_block & 15) return fail(ANTSRL_E_INVALID, "checkpoint_save: device_block must be 16-byte aligned");
    EnvCopyTable t;
    if (int rc = ckpt_table(h, &t, (unsigned char *)device_block, true, "checkpoint_save")) return rc;
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc; // (the block holds the state BEHIND a deferred update)
    if (int rc = enqueued(antsrl_launch_env_copy(t, (hipStream_t)stream), "checkpoint_save")) return rc;
    AntsCkptBlob b;
    memset(&b, 0, sizeof(b));
    b.magic = ANTSRL_CKPT_MAGIC; b.version = ANTSRL_CKPT_VERSION; b.size = sizeof(b);
    b.cfg = h->cfg;
    b.cur = h->cur; b.steps_since_update = h->steps_since_update; b.host_timestep = h->host_timestep;
    b.obs_seq = h->obs_seq; b.sum_obs = h->sum_obs;
    b.need_full_collect = h->need_full_collect; b.is_reset = h->is_reset; b.episode_over = h->episode_over;
    b.has_gen = h->has_gen && h->gen.wall_kind != ANTSRL_WALLS_INPUT; // (its bitmaps are the caller's: not carried)
    b.sum_due = h->sum_due; b.sum_live = h->sum_live; b.need_wall_clear = h->need_wall_clear;
    b.sweeps = h->sweeps; b.episode_seed = h->episode_seed; b.deposit_strength = h->p.deposit_strength;
    if (b.has_gen) {
        b.gen = h->gen;
        b.gen.walls_input = nullptr;
    }
    memcpy(host_blob, &b, sizeof(b));
    return ANTSRL_OK;
}

extern "C" int antsrl_checkpoint_load(AntsHandle *h, const void *device_block, const void *host_blob, void *stream)
{
    if (!h || !device_block || !host_blob) return fail(ANTSRL_E_INVALID, "checkpoint_load: NULL handle, device_block or host_blob");
    AntsCkptBlob b;
    memcpy(&b, host_blob, 16); // magic, version, size: the rest only once these say what it is
    if (b.magic != ANTSRL_CKPT_MAGIC) return fail(ANTSRL_E_INVALID, "checkpoint_load: host_blob has magic 0x%08x, not 0x%08x", b.magic, ANTSRL_CKPT_MAGIC);
    if (b.version != ANTSRL_CKPT_VERSION)
        return fail(ANTSRL_E_INVALID, "checkpoint_load: host_blob has format version %u, this library reads %u", b.version, ANTSRL_CKPT_VERSION);
    if (b.size != sizeof(b)) return fail(ANTSRL_E_INVALID, "checkpoint_load: host_blob says size %llu, the format's is %zu", (unsigned long long)b.size, sizeof(b));
    memcpy(&b, host_blob, sizeof(b));
    const unsigned char *theirs = (const unsigned char *)&b.cfg, *ours = (const unsigned char *)&h->cfg;
    for (size_t i = 0; i < sizeof(AntsCfg); ++i)
        if (theirs[i] != ours[i])
            return fail(ANTSRL_E_INVALID, "checkpoint_load: the checkpoint's AntsCfg differs from this handle's in %s (byte %zu)", cfg_field_at(i), i);
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if ((uintptr_t)device_block & 15) return fail(ANTSRL_E_INVALID, "checkpoint_load: device_block must be 16-byte aligned");
    EnvCopyTable t;
    if (int rc = ckpt_table(h, &t, (unsigned char *)device_block, false, "checkpoint_load")) return rc;
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc; // (ahead of the copy that replaces what it writes)
    if (int rc = enqueued(antsrl_launch_env_copy(t, (hipStream_t)stream), "checkpoint_load")) return rc;
    h->cur = b.cur; h->steps_since_update = b.steps_since_update; h->host_timestep = b.host_timestep;
    h->obs_seq = b.obs_seq; h->sum_obs = b.sum_obs;
    h->need_full_collect = b.need_full_collect; h->is_reset = b.is_reset; h->episode_over = b.episode_over;
    h->sum_due = b.sum_due; h->need_wall_clear = b.need_wall_clear;
    h->sweeps = b.sweeps; h->episode_seed = b.episode_seed; h->p.deposit_strength = b.deposit_strength;
    h->has_gen = b.has_gen;
    if (b.has_gen) h->gen = b.gen;
    set_decay(h); // g_now / g_dep / inv_g_dep follow from sweeps
    // The summary's bits came over with explored_bits.  A set bit is a fact about the explored stamps, which came over with
    // the records (antsrl_explored.h): it stays true in any handle, so one that keeps a summary goes on consuming it.
    h->sum_live = b.sum_live && summary_on(h);
    return ANTSRL_OK;
}

extern "C" int antsrl_fork_envs(AntsHandle *h, const int32_t *src, const int32_t *dst, int32_t n, void *stream)
{
    if (!h || !src || !dst) return fail(ANTSRL_E_INVALID, "fork_envs: NULL handle, src or dst");
    if (n < 1) return fail(ANTSRL_E_INVALID, "fork_envs: n must be >= 1, got %d", n);
    const int32_t E = h->p.E;
    uint32_t is_dst[(65535 + 31) / 32 + 1];
    memset(is_dst, 0, sizeof(is_dst));
    for (int32_t i = 0; i < n; ++i) { // (stops at the first repeated dst: at most E + 1 entries are read)
        if (src[i] < 0 || src[i] >= E) return fail(ANTSRL_E_INVALID, "fork_envs: src[%d] = %d is not in [0, %d)", i, src[i], E);
        if (dst[i] < 0 || dst[i] >= E) return fail(ANTSRL_E_INVALID, "fork_envs: dst[%d] = %d is not in [0, %d)", i, dst[i], E);
        if (is_dst[dst[i] >> 5] >> (dst[i] & 31) & 1u) return fail(ANTSRL_E_INVALID, "fork_envs: dst %d appears twice (dst[%d])", dst[i], i);
        is_dst[dst[i] >> 5] |= 1u << (dst[i] & 31);
    }
    for (int32_t i = 0; i < n; ++i)
        if (is_dst[src[i] >> 5] >> (src[i] & 31) & 1u)
            return fail(ANTSRL_E_INVALID, "fork_envs: environment %d is a src (src[%d]) and a dst", src[i], i);
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    EnvCopyTable t;
    if (int rc = ckpt_table(h, &t, nullptr, false, "fork_envs")) return rc;
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc;
    for (int32_t i0 = 0; i0 < n; i0 += ENV_COPY_MAX_PAIRS) { // (the pairs are kernel arguments: one launch per 640 of them)
        t.rows = n - i0 < ENV_COPY_MAX_PAIRS ? n - i0 : ENV_COPY_MAX_PAIRS;
        for (int32_t i = 0; i < t.rows; ++i) {
            t.pair_src[i] = (uint16_t)src[i0 + i];
            t.pair_dst[i] = (uint16_t)dst[i0 + i];
        }
        if (int rc = enqueued(antsrl_launch_env_copy(t, (hipStream_t)stream), "fork_envs")) return rc;
    }
    return ANTSRL_OK;
}

extern "C" int antsrl_step_update(AntsHandle *h, const int8_t *rotation, const int8_t *phero,
                                  const double *wall_jitter, float *obs, float *agent_state, float *reward,
                                  uint8_t *done, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if (!agent_state || !reward || !done) return fail(ANTSRL_E_INVALID, "agent_state, reward, done are required");
    hipStream_t st = (hipStream_t)stream;
    const bool timed = h->ev_armed;
    h->ev_armed = false;
    if (timed) (void)hipEventRecord(h->ev[0], st);
    // The sweep only reads phero[cur] and the wall bitmap, so it can be enqueued first: the
    // perception gather of the step reads the same (pre-update) buffer.  Except behind a DEFERRED update: its deposits land
    // in phero[cur] — this sweep's input — with k_update_move, so the sweep follows the step's kernels (the perception
    // reads phero[cur], too, and nothing of the step reads the sweep's output).
    const bool sweep_late = !h->p.scaled && h->pend_update;
    if (!h->p.scaled && !sweep_late)
        if (int rc = enqueued(antsrl_launch_sweep(h->p, h->cur, st), "pheromone sweep")) return rc;
    if (timed) (void)hipEventRecord(h->ev[1], st);
    int rc = do_step(h, rotation, phero, obs, agent_state, reward, done, st, timed);
    if (rc) return rc;
    if (timed) (void)hipEventRecord(h->ev[3], st);
    rc = summary_refresh_due(h, st);
    if (rc) return rc;
    if (sweep_late) rc = enqueued(antsrl_launch_sweep(h->p, h->cur, st), "pheromone sweep");
    if (rc) return rc;
    const bool was_done = h->host_timestep == h->cfg.max_time; // RL_api.py:200, same for every env
    const bool regen = was_done && h->has_gen && h->gen.auto_reset;
    rc = do_update(h, wall_jitter, st, true, !regen);
    if (timed) (void)hipEventRecord(h->ev[4], st);
    if (rc == ANTSRL_OK && regen) {
        // next episode, like main.py:69-79 does per episode (reference streams: global env g takes seed + g, so the next
        // episode starts one whole batch — AntsCfg.n_envs_total, all shards — of seeds further)
        const uint64_t total = h->cfg.n_envs_total ? (uint64_t)h->cfg.n_envs_total : (uint64_t)h->p.env_id_base + (uint64_t)h->p.E;
        rc = do_generate(h, h->episode_seed + (h->gen.rng_kind == ANTSRL_RNG_REFERENCE ? total : 1u), st);
        if (rc != ANTSRL_OK) {
            // The step and the update have run, the next episode could not be drawn (the 32-bit seed limit): the handle
            // holds a finished episode.  Every later step fails loudly until antsrl_reset / antsrl_generate gives it a
            // new one, instead of running past max_time with `done` never firing again.
            h->is_reset = false;
            h->episode_over = true;
        }
    }
    return rc;
}

extern "C" int antsrl_query(const AntsHandle *h, int what, long long *value)
{
    if (!h || !value) return fail(ANTSRL_E_INVALID, "NULL handle or value");
    switch (what) {
    case ANTSRL_Q_CELL_META: *value = h->p.meta; break;
    case ANTSRL_Q_SCALED_UNITS: *value = h->p.scaled; break;
    case ANTSRL_Q_INTERLEAVED: *value = h->p.ps == 4 && h->p.fs == 4; break;
    case ANTSRL_Q_FILTER_SEPARABLE: *value = h->p.filter_sep; break;
    case ANTSRL_Q_PERCEIVE_RUN: *value = h->p.meta ? antsrl_perceive_run(h->p) : 0; break;
    case ANTSRL_Q_TIMESTEP: *value = h->host_timestep; break;
    case ANTSRL_Q_DEFERRED_UPDATE: *value = antsrl_update_move_supported(h->p); break;
    case ANTSRL_Q_PERCEIVE_FAST: *value = h->p.meta && !h->prc_generic && antsrl_perceive_fast(h->p); break;
    case ANTSRL_Q_EXPLORED_SUMMARY: *value = summary_on(h); break;
    default: return fail(ANTSRL_E_INVALID, "bad query selector %d", what);
    }
    return ANTSRL_OK;
}

extern "C" int antsrl_bench_copy(void *dst, const void *src, size_t bytes, void *stream)
{
    if (!dst || !src || (bytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15))
        return fail(ANTSRL_E_INVALID, "bench_copy: 16-byte aligned pointers and a multiple of 16 bytes");
    return enqueued(antsrl_launch_copy16(dst, src, bytes, (hipStream_t)stream), "bench_copy");
}

extern "C" int antsrl_set_timing_events(AntsHandle *h, void *const *events)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    h->ev_armed = events != nullptr;
    if (events)
        for (int i = 0; i < ANTSRL_TIMING_EVENTS; ++i) h->ev[i] = (hipEvent_t)events[i];
    return ANTSRL_OK;
}

extern "C" int antsrl_set_activation(AntsHandle *h, const float *act, double new_deposit_strength, void *stream)
{
    if (!h || !act) return fail(ANTSRL_E_INVALID, "NULL handle or act");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc; // (the deferred update deposits with the activation as it was)
    if (int rc = enqueued(antsrl_launch_set_activation(h->p, act, (hipStream_t)stream), "set_activation")) return rc;
    if (new_deposit_strength > 0) h->p.deposit_strength = new_deposit_strength;
    return ANTSRL_OK;
}

extern "C" int antsrl_policy_mlp(AntsHandle *h, const float *obs, const float *agent_state, int64_t n_ants,
                                 int32_t n_features, const float *w1, const float *b1, const float *w2,
                                 const float *b2, const float *w3, const float *b3, int8_t *rotation,
                                 int8_t *pheromone, float *logits, void *stream)
{
    // h may be NULL (float32 observations); a handle supplies the observation format (antsrl_set_obs_format)
    if (!obs || !agent_state || !w1 || !b1 || !w2 || !b2 || !rotation)
        return fail(ANTSRL_E_INVALID, "policy_mlp: obs, agent_state, w1, b1, w2, b2, rotation are required");
    if ((w3 == nullptr) != (b3 == nullptr) || (pheromone && !w3))
        return fail(ANTSRL_E_INVALID, "policy_mlp: w3/b3 go together and are needed for a pheromone output");
    if (n_ants < 1 || n_ants > 0x7fffffff || n_features < 1 || n_features + 2 > 1024)
        return fail(ANTSRL_E_INVALID, "policy_mlp: n_ants >= 1 and 1 <= n_features <= 1022");
    return enqueued(antsrl_launch_policy(obs, agent_state, w1, b1, w2, b2, w3, b3, rotation, pheromone, logits, (int)n_ants,
                                         n_features, (hipStream_t)stream, h && h->obs_bf16),
                    "policy_mlp");
}

extern "C" int antsrl_set_inloop_policy(AntsHandle *h, int32_t n_features, const float *w1, const float *b1, const float *w2,
                                        const float *b2, const float *w3, const float *b3, int8_t *rotation_next,
                                        int8_t *pheromone_next, void *stream)
{
    if (!h) return fail(ANTSRL_E_INVALID, "NULL handle");
    if (!w1) { // switch it off
        h->pol = PolArgs{};
        return ANTSRL_OK;
    }
    if (!b1 || !w2 || !b2 || !rotation_next)
        return fail(ANTSRL_E_INVALID, "inloop_policy: w1, b1, w2, b2, rotation_next are required");
    if ((w3 == nullptr) != (b3 == nullptr) || (pheromone_next && !w3))
        return fail(ANTSRL_E_INVALID, "inloop_policy: w3/b3 go together and are needed for a pheromone output");
    if (n_features != h->p.PP * h->p.K)
        return fail(ANTSRL_E_INVALID, "inloop_policy: n_features must be P*P*K = %d", h->p.PP * h->p.K);
    if (!h->obs_bf16 || !antsrl_inloop_policy_supported(h->p))
        return fail(ANTSRL_E_UNSUPPORTED, "inloop_policy needs the cell-meta path (ANTSRL_Q_CELL_META) with bfloat16 "
                                          "observations (antsrl_set_obs_format) — use antsrl_policy_mlp otherwise");
    if (h->obs_pitch != 0 && h->obs_pitch != (uint32_t)(h->p.PP * h->p.K))
        return fail(ANTSRL_E_UNSUPPORTED, "the in-loop policy and a padded observation row stride exclude each other (the net reads a "
                                          "dense tile image): antsrl_set_obs_row_stride(h, 0) first");
    if (int rc = enqueued(antsrl_launch_policy_pack(h->p.s.pol_pack, w1, b1, w2, b2, w3, b3, n_features, (hipStream_t)stream),
                          "inloop_policy pack"))
        return rc;
    h->pol.pack = h->p.s.pol_pack;
    h->pol.rot = rotation_next;
    h->pol.ph = pheromone_next;
    h->pol.ks = (n_features + 15) / 16;
    return ANTSRL_OK;
}

static size_t state_bytes(const AntsHandle *h, int which)
{
    const size_t E = h->p.E, N = h->p.N, G = (size_t)h->p.W * h->p.H, C = h->p.C, R = h->p.R;
    switch (which) {
    case ANTSRL_S_ANTS_XYT: return 8 * E * N * 3;
    case ANTSRL_S_PREV_XY: return 8 * E * N * 2;
    case ANTSRL_S_HOLDING: case ANTSRL_S_SEED: return 4 * E * N;
    case ANTSRL_S_MANDIBLES: case ANTSRL_S_REWARD_STATE: return E * N;
    case ANTSRL_S_ACTIVATION: return 4 * E * N * C;
    case ANTSRL_S_PHERO: return 4 * E * C * G;
    case ANTSRL_S_FOOD: return 4 * E * G;
    case ANTSRL_S_EXPLORED: case ANTSRL_S_WALLS: case ANTSRL_S_ANTHILL_AREA: return E * G;
    case ANTSRL_S_ANTHILL_FOOD: return 8 * E;
    case ANTSRL_S_ROCK_CENTERS: return 8 * E * R * 2;
    case ANTSRL_S_TIMESTEP: return 4 * E;
    case ANTSRL_S_ANTHILL_XYR: return 4 * E * 3;
    case ANTSRL_S_ROCK_RW: return 8 * E * R * 2;
    case ANTSRL_S_PHERO_C0: case ANTSRL_S_PHERO_C1: case ANTSRL_S_PHERO_C2: case ANTSRL_S_PHERO_C3:
        return (size_t)(which - ANTSRL_S_PHERO_C0) < C ? 4 * E * G : 0;
    default: return 0;
    }
}

extern "C" int antsrl_state_bytes(const AntsHandle *h, int which, size_t *bytes)
{
    if (!h || !bytes) return fail(ANTSRL_E_INVALID, "NULL handle or bytes");
    if (which < 0 || which >= ANTSRL_S_COUNT_) return fail(ANTSRL_E_INVALID, "bad state selector %d", which);
    *bytes = state_bytes(h, which);
    return ANTSRL_OK;
}

extern "C" int antsrl_perceptive_field(AntsHandle *h, uint8_t *dst, void *stream)
{
    if (!h || !dst) return fail(ANTSRL_E_INVALID, "NULL handle or dst");
    if (int rc = handle_ready(h, MID_UPDATE_ALLOWED)) return rc;
    // (no flush: a DEFERRED update has not touched the positions yet — the field is the last observation's, as in the
    //  reference, where RLApi.observation computes it; behind an update that has run it is the moved ants')
    return enqueued(antsrl_launch_perceptive_field(h->p, dst, (hipStream_t)stream), "perceptive_field");
}

// A caller's Reward (include/antsrl.h): obs_coords for its observation(), give_reward for what its step() returned.  Both
// sit between the step and the update; behind a DEFERRED update they enqueue it first — give_reward's 255 must land on
// the decayed reward_state, and the coordinates are those of the ants where the update left them.
extern "C" int antsrl_obs_coords(AntsHandle *h, int32_t *dst, void *stream)
{
    if (!h || !dst) return fail(ANTSRL_E_INVALID, "NULL handle or dst");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if ((uintptr_t)dst & 7) return fail(ANTSRL_E_INVALID, "obs_coords: dst must be 8-byte aligned (one int32 pair per store)");
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc;
    return enqueued(antsrl_launch_obs_coords(h->p, dst, (hipStream_t)stream), "obs_coords");
}

extern "C" int antsrl_give_reward(AntsHandle *h, const double *reward, double threshold, float *reward_out, void *stream)
{
    if (!h || !reward) return fail(ANTSRL_E_INVALID, "NULL handle or reward");
    if (int rc = handle_ready(h, MID_UPDATE_REFUSED)) return rc;
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc;
    return enqueued(antsrl_launch_give_reward(h->p, reward, threshold, reward_out, (hipStream_t)stream), "give_reward");
}

extern "C" int antsrl_read_state(AntsHandle *h, int which, void *dst, void *stream)
{
    if (!h || !dst) return fail(ANTSRL_E_INVALID, "NULL handle or dst");
    if (int rc = handle_ready(h, MID_UPDATE_ALLOWED)) return rc;
    if (which < 0 || which >= ANTSRL_S_COUNT_) return fail(ANTSRL_E_INVALID, "bad state selector %d", which);
    if (state_bytes(h, which) == 0) return ANTSRL_OK;
    if (int rc = flush_pending(h, (hipStream_t)stream)) return rc;
    return enqueued(antsrl_launch_read_state(h->p, which, h->cur, dst, (hipStream_t)stream), "read_state");
}
