/*
 * antsrl.h — C-ABI of libantsrl_hip.so: the MI355X (gfx950) implementation of the
 * AntsRL environment step loop (RLApi.step + Environment.update), batched over
 * many independent environments.
 *
 * The reference (SelennLamson/AntsRL) is pure Python and has no FFI of its own:
 * the boundary it exposes is the Python surface of `RLApi` / `Environment`
 * (SURVEY.md §8(b)).  Each entry point below names the reference interface it
 * replaces (paths relative to the reference checkout).  The Python shim
 * `antsrl_amd.RLApi` binds these through ctypes, passing `tensor.data_ptr()`
 * of torch-ROCm tensors; INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - plain C types only; every buffer is caller-owned DEVICE memory, env-major
 *    and contiguous; the library never allocates, frees or synchronises inside
 *    step/update/observe (it only enqueues kernels on the caller's stream);
 *  - all persistent state lives in ONE caller-provided device workspace whose
 *    size is reported by antsrl_workspace_bytes() — or in two blocks, cell records
 *    and everything else (antsrl_workspace_bytes2 / antsrl_create2);
 *  - return value 0 = success, negative = error (see ANTSRL_E_*); nothing is
 *    thrown across the ABI; antsrl_last_error() gives a message for the last
 *    failure on the calling thread;
 *  - a handle belongs to the device its workspace lives on (any number of handles per device), holds up
 *    to 65535 environments and is not thread-safe;
 *  - sizes: any grid; up to 4096 ants per env with the reference's perception shapes (2 pheromone channels,
 *    the generator's channel order, up to 64 perceived cells: the cell-meta path, k_move + k_perceive),
 *    ~2400 with other channel lists (k_act keeps per-ant frames in LDS); antsrl_create() returns
 *    ANTSRL_E_UNSUPPORTED beyond that.
 */
#ifndef ANTSRL_H
#define ANTSRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANTSRL_ABI_VERSION 5

#define ANTSRL_MAX_CHANNELS 16
#define ANTSRL_MAX_PSIDE 15                                      /* 2*radius+1 <= 15 */
#define ANTSRL_MAX_PCELLS (ANTSRL_MAX_PSIDE * ANTSRL_MAX_PSIDE)
#define ANTSRL_MAX_FILTER_RADIUS 3
#define ANTSRL_MAX_FILTER_TAPS 49
#define ANTSRL_MAX_PHERO 4

/* error codes */
#define ANTSRL_OK 0
#define ANTSRL_E_INVALID (-1)   /* bad argument / configuration */
#define ANTSRL_E_NOMEM (-2)     /* workspace too small */
#define ANTSRL_E_DEVICE (-3)    /* HIP runtime error (launch / no device) */
#define ANTSRL_E_UNSUPPORTED (-4)

/* perceived-object kinds: one perception channel per entry of
 * RLApi.perceived_objects (environment/RL_api.py:123-142) */
enum {
    ANTSRL_CH_ANTS = 0,    /* RL_api.py:136-142  presence 0/1            */
    ANTSRL_CH_PHERO = 1,   /* RL_api.py:124-125  phero/max_val (arg = i) */
    ANTSRL_CH_ANTHILL = 2, /* RL_api.py:130-131  area                    */
    ANTSRL_CH_WALLS = 3,   /* RL_api.py:128-129  map                     */
    ANTSRL_CH_FOOD = 4,    /* RL_api.py:126-127  qte                     */
    ANTSRL_CH_ROCKS = 5    /* RL_api.py:132-135  any(dist < radius)      */
};

/* Pheromone.update strategy.  With the shipped centre-only DIFFUSE_FILTER (DIFFUSE_FACTOR = 0,
 * pheromone.py:5-10) the update is a per-cell multiply by f0 = 1 - EVAP_FACTOR plus a cut at
 * 0.01.  AUTO then stores the grid in units of f0^S (S = updates so far), so evaporation costs no
 * per-step pass over the grid at all; values are materialised (v = u * f0^S, zero below the cut)
 * wherever they are read.  EXPLICIT_SWEEP forces the streaming sweep kernel (k_sweep0); filters with a
 * radius always take an explicit per-step sweep: a register-marching stencil (k_sweep_r1x2 / k_sweep_sep2 /
 * k_sweep_march). */
enum { ANTSRL_PHERO_AUTO = 0, ANTSRL_PHERO_EXPLICIT_SWEEP = 1 };

/* Which kernels run RLApi.step / RLApi.observation.  AUTO picks by measurement: the cell-meta path (k_move +
 * k_perceive) wherever it is supported (the generator's channel order, two pheromone channels, a perception of 128..368
 * values per ant, at most 4096 ants per environment), the single kernel k_act elsewhere.  The other two values pin a
 * path (antsrl_create refuses a configuration the pinned path does not support): results are identical, both are
 * parity-tested. */
enum { ANTSRL_ACT_AUTO = 0, ANTSRL_ACT_CELL_META = 1, ANTSRL_ACT_SINGLE_KERNEL = 2 };

/* reward kinds (environment/rewards/) */
enum {
    ANTSRL_REWARD_NONE = 0,        /* Reward base: zeros, reward.py:19,38       */
    ANTSRL_REWARD_EXPLORATION = 1, /* ExplorationReward, reward_custom.py:8-25  */
    ANTSRL_REWARD_FOOD = 2,        /* Food_Reward, reward_custom.py:28-40       */
    ANTSRL_REWARD_ALL = 3          /* All_Rewards, reward_custom.py:43-109      */
};

/* Static configuration of a batch of environments.  Gathers the constructor
 * arguments and module constants the reference spreads over RLApi.__init__
 * (RL_api.py:23), RLApi.setup_perception (RL_api.py:80-93), DELTA (RL_api.py:15),
 * EnvironmentGenerator.__init__ (generator/environment_generator.py:20-46),
 * Ants.__init__ (ants.py:18), Pheromone (pheromone.py:5-10,21) and the reward
 * constructors (rewards/reward_custom.py:44). */
typedef struct AntsCfg {
    int32_t abi_version; /* = ANTSRL_ABI_VERSION */
    int32_t n_envs;      /* E : independent environments in this batch   */
    int32_t n_ants;      /* N : ants per environment                      */
    int32_t w, h;        /* grid; cell (x,y) is element [x][y], y fastest */
    int32_t n_phero;     /* C : pheromone channels (<= ANTSRL_MAX_PHERO)  */
    int32_t n_rocks;     /* R : circle obstacles per env (0 = none)       */
    int32_t max_time;    /* Environment.max_time, environment.py:26       */

    /* perception (RLApi.setup_perception) */
    int32_t perception_radius;                  /* r, side P = 2r+1             */
    int32_t n_channels;                         /* K = len(perceived_objects)   */
    int32_t channel_kind[ANTSRL_MAX_CHANNELS];  /* ANTSRL_CH_*                  */
    int32_t channel_arg[ANTSRL_MAX_CHANNELS];   /* pheromone index for CH_PHERO */
    int32_t has_mask;                           /* 0: perception_mask is None   */
    uint8_t mask[ANTSRL_MAX_PCELLS];            /* [P][P] row-major, 1=visible  */
    uint8_t _pad0[7];
    double delta;     /* DELTA = 1.1, RL_api.py:15                      */
    double fwd_delta; /* perception_shift = 4, environment_generator.py:43 */

    /* kinematics (RLApi.__init__, main.py:45-50) */
    double max_speed, max_rot_speed, carry_speed_reduction, backward_speed_reduction;
    double max_hold; /* Ants.max_hold = 5, environment_generator.py:93 */

    /* pheromone (pheromone.py:5-10, 36-45) */
    int32_t has_max_val;      /* Pheromone.max_val is not None                   */
    int32_t filter_radius;    /* 0..3 ; DIFFUSE_FILTER side = 2*radius+1         */
    double phero_max_val;     /* 255                                             */
    double deposit_strength;  /* what activate_pheromone's 256 becomes: 1.0 while
                                 phero_activation is bool (ants.py:83), 256.0 once
                                 an agent called activate_all_pheromones(float)   */
    double phero_threshold;   /* 0.01, pheromone.py:45                           */
    double filter[ANTSRL_MAX_FILTER_TAPS]; /* DIFFUSE_FILTER [side][side] row-major
                                 (first index along x), applied as scipy's
                                 convolve2d(.., 'same', 'fill', 0), pheromone.py:44 */

    /* reward */
    int32_t reward_kind; /* ANTSRL_REWARD_* */
    int32_t phero_mode;  /* ANTSRL_PHERO_AUTO (0) or ANTSRL_PHERO_EXPLICIT_SWEEP (1), see below */
    double reward_threshold; /* RLApi.reward_threshold, RL_api.py:32,203 */
    double fct_explore, fct_food, fct_anthill, fct_explore_holding, fct_headinganthill;

    /* Walls.update jitter (walls.py:28) when no explicit draws are supplied:
     * counter-based generator keyed on (rng_seed, GLOBAL env id, timestep, ant). */
    uint64_t rng_seed;

    int32_t act_path; /* ANTSRL_ACT_* (no reference counterpart) */

    /* GLOBAL ENVIRONMENT IDENTITY (ABI 5).  The reference seeds every environment by itself
     * (generator/environment_generator.py:53-55; the np.random stream Walls.update draws from, walls.py:28, belongs
     * to that environment), so an environment's trajectory must not depend on which handle / rank / batch position
     * it lands on.  Environment e of this handle IS global environment env_id_base + e: every random stream the
     * library keys on an environment — the built-in wall jitter, both generators of antsrl_generate — takes the
     * global id.  A handle over envs [lo, hi) of a sharded batch with env_id_base = lo reproduces rows lo:hi of the
     * whole-batch handle bit for bit (tests/test_gpu_shard_identity.py).  n_envs_total: environments in the whole
     * (sharded) batch, the stride between the auto-reset episodes of ANTSRL_RNG_REFERENCE (env g of episode k draws
     * from episode_seed + k * n_envs_total + g); 0 = env_id_base + n_envs. */
    int32_t env_id_base;
    int32_t n_envs_total;
    int32_t _pad1;
} AntsCfg;

/* Initial state of every environment = what EnvironmentGenerator.generate
 * (generator/environment_generator.py:52-106) builds.  All device pointers. */
typedef struct AntsInit {
    const double *ants_xyt;    /* [E][N][3]  Ants.ants, ants.py:27              */
    const double *seed;        /* [E][N]     Ants.seed, ants.py:41              */
    const uint8_t *walls;      /* [E][W][H]  Walls.map, walls.py:14             */
    const float *food;         /* [E][W][H]  Food.qte, food.py:15               */
    const int32_t *anthill_xyr;/* [E][3]     Anthill x,y,radius, anthill.py:17  */
    const double *rocks;       /* [E][R][4]  cx,cy,radius,weight (NULL if R=0),
                                              circle_obstacles.py:16             */
    const float *phero;        /* [E][C][W][H] or NULL (= zeros), pheromone.py:28-31 */
} AntsInit;

/* Parameters of the device-side episode generator (antsrl_generate): the knobs of
 * EnvironmentGenerator.__init__ / CirclesGenerator (generator/environment_generator.py:20-46,
 * generator/map_generators.py:28-33, main.py:70-77) that are not already in AntsCfg. */
#define ANTSRL_MAX_FOOD_DISCS 64
#define ANTSRL_WALLS_BERNOULLI 0 /* independent wall cells with probability wall_density */
#define ANTSRL_WALLS_PERLIN 1    /* PerlinGenerator (generator/map_generators.py:9-25, main.py:75):
                                    wall = pnoise2((x + ox) / scale, (y + oy) / scale, octaves, persistence,
                                    lacunarity) > wall_density, per-env offsets ox, oy uniform in
                                    [-10000, 10000]; improved Perlin noise restated from the published
                                    algorithm in float32 (the `noise` package is absent: unpinned) */
#define ANTSRL_WALLS_INPUT 2     /* the caller's bitmap (AntsGen.walls_input, uint8 [E][W][H], device memory): what any
                                    walls_generator.generate(w, h) returned; cleared on the anthill area
                                    like environment_generator.py:66-67 */
/* random streams of the device generator */
#define ANTSRL_RNG_COUNTER 0     /* counter-based, keyed on (episode_seed, global env id, item): same distributions as
                                    the reference's generator, different maps (the oracle restates it) */
#define ANTSRL_RNG_REFERENCE 1   /* the reference's own streams: env e (global id g = AntsCfg.env_id_base + e) is drawn
                                    like EnvironmentGenerator(seed = episode_seed + g).generate — random.seed(seed) / np.random.seed(seed * 5)
                                    (environment_generator.py:53-55), i.e. two MT19937 generators per env with
                                    Python's and numpy's seeding and 53-bit doubles, consumed in the reference's order
                                    (anthill :60-63, PerlinGenerator's two randints map_generators.py:19-20,
                                    CirclesGenerator :37-39, rocks :77-85, ants :87-91, Ants.seed ants.py:41): equal
                                    seeds give the reference's anthill, food discs, ants and seeds bit for bit.
                                    Walls: ANTSRL_WALLS_PERLIN or ANTSRL_WALLS_INPUT.
                                    (episode_seed + env_id_base + E) * 5 < 2^32. */
typedef struct AntsGen {
    double wall_density;   /* Bernoulli: probability of a wall cell; Perlin: PerlinGenerator.density (threshold) */
    int32_t n_food_discs;  /* CirclesGenerator.n_circles, main.py:74 uses 20 (<= ANTSRL_MAX_FOOD_DISCS) */
    int32_t food_rmin, food_rmax; /* CirclesGenerator min/max radius, main.py:74 uses 5, 10 */
    int32_t auto_reset;    /* 1: antsrl_step_update regenerates every env right after the update of
                              the step that reported done (RL_api.py:200), with the next episode seed */
    int32_t wall_kind;     /* ANTSRL_WALLS_* */
    int32_t perlin_octaves;      /* PerlinGenerator defaults: 2 (1..8) */
    double perlin_scale;         /* 22.0 */
    double perlin_persistence;   /* 0.5 */
    double perlin_lacunarity;    /* 2.0 */
    int32_t rng_kind;            /* ANTSRL_RNG_* */
    int32_t _pad;
    const uint8_t *walls_input;  /* ANTSRL_WALLS_INPUT: uint8 [E][W][H] device memory, else NULL */
} AntsGen;

typedef struct AntsHandle AntsHandle;

/* selectors for antsrl_read_state: canonical (reference-shaped) layouts */
enum {
    ANTSRL_S_ANTS_XYT = 0,     /* double  [E][N][3]                     */
    ANTSRL_S_PREV_XY = 1,      /* double  [E][N][2]   Ants.prev_ants    */
    ANTSRL_S_HOLDING = 2,      /* float   [E][N]                        */
    ANTSRL_S_MANDIBLES = 3,    /* uint8   [E][N]                        */
    ANTSRL_S_ACTIVATION = 4,   /* float   [E][N][C]   phero_activation  */
    ANTSRL_S_PHERO = 5,        /* float   [E][C][W][H]                  */
    ANTSRL_S_FOOD = 6,         /* float   [E][W][H]                     */
    ANTSRL_S_EXPLORED = 7,     /* uint8   [E][W][H]   reward explored_map */
    ANTSRL_S_ANTHILL_FOOD = 8, /* double  [E]         Anthill.food      */
    ANTSRL_S_ROCK_CENTERS = 9, /* double  [E][R][2]                     */
    ANTSRL_S_TIMESTEP = 10,    /* int32   [E]                           */
    ANTSRL_S_REWARD_STATE = 11,/* uint8   [E][N]      Ants.reward_state */
    ANTSRL_S_WALLS = 12,       /* uint8   [E][W][H]                     */
    ANTSRL_S_ANTHILL_AREA = 13,/* uint8   [E][W][H]   Anthill.area      */
    ANTSRL_S_SEED = 14,        /* float   [E][N]                        */
    ANTSRL_S_ANTHILL_XYR = 15, /* int32   [E][3]      Anthill.x, .y, .radius (anthill.py:21-23) */
    ANTSRL_S_ROCK_RW = 16,     /* double  [E][R][2]   CircleObstacles.radiuses, .weights (circle_obstacles.py:19-20) */
    ANTSRL_S_PHERO_C0 = 17,    /* float   [E][W][H]   one pheromone channel: Pheromone.phero of pheromone 0 ...   */
    ANTSRL_S_PHERO_C1 = 18,    /*                     ... 1 (a view of ONE Pheromone object reads one channel,    */
    ANTSRL_S_PHERO_C2 = 19,    /*                     not all of them)                                            */
    ANTSRL_S_PHERO_C3 = 20,
    ANTSRL_S_COUNT_
};

/* Library / ABI version (ANTSRL_ABI_VERSION of the build). */
int antsrl_abi_version(void);

/* sizeof(AntsCfg) as the library was compiled: lets a binding verify its struct mirror. */
size_t antsrl_cfg_size(void);

/* Message for the last error returned on this thread ("" if none). */
const char *antsrl_last_error(void);

/* Bytes of device workspace a batch with this configuration needs.
 * No reference counterpart (the reference allocates numpy arrays per object). */
int antsrl_workspace_bytes(const AntsCfg *cfg, size_t *bytes);

/* Creates a handle over a caller-owned device workspace (>= workspace_bytes,
 * 256-byte aligned).  Replaces RLApi.__init__ (environment/RL_api.py:23) +
 * RLApi.setup_perception (RL_api.py:80-93).  Host-only: touches no device state. */
int antsrl_create(const AntsCfg *cfg, void *workspace, size_t workspace_bytes, AntsHandle **out);

/* The workspace as TWO caller-provided blocks (no reference counterpart).  The RECORD block holds what the kernels reach
 * with scattered per-cell accesses: the interleaved {p0, p1, food, META} cell records, or — any other configuration — the
 * pheromone buffers and the food / {food, META} records.  The STATE block holds everything else: the per-ant and per-env
 * arrays (streamed), the bit maps, the perception frames, the rock tables, the generator's tables and the in-loop policy's
 * pack.  On MI355X a scattered stream and a streaming one run slower against each other inside one zone of the device's
 * memory than across two: with two blocks the caller can place them apart, which one block — one
 * allocation, one zone — cannot.  The blocks may lie anywhere relative to each other (either may have the lower address);
 * each is 256-byte aligned and must not overlap the other.  antsrl_workspace_bytes2 reports the two sizes (either pointer
 * may be NULL); their sum equals antsrl_workspace_bytes.  A handle of antsrl_create2 behaves exactly like one of
 * antsrl_create in every entry point, bit for bit; antsrl_create is antsrl_create2 over one block, carved in one sequence
 * (the records between the per-ant arrays and the bit maps, where they have always been). */
int antsrl_workspace_bytes2(const AntsCfg *cfg, size_t *state_bytes, size_t *record_bytes);
int antsrl_create2(const AntsCfg *cfg, void *state_ws, size_t state_bytes, void *record_ws, size_t record_bytes,
                   AntsHandle **out);

/* Where every array of the workspace lies (host only; no reference counterpart: tests and tools check the carve with it).
 * split = 0: the one block of antsrl_create (block is 0 for every entry); split = 1: the two blocks of antsrl_create2
 * (block 0 = state, 1 = records).  Writes min(*count, cap) entries in carve order and sets *count to the number of arrays
 * (entries may be NULL with cap 0).  An entry's reserved bytes are `bytes` rounded up to 256. */
typedef struct AntsWsArray {
    char name[24];
    int32_t block, _pad;
    uint64_t offset, bytes;
} AntsWsArray;
int antsrl_workspace_map(const AntsCfg *cfg, int split, AntsWsArray *entries, int32_t cap, int32_t *count);

void antsrl_destroy(AntsHandle *h);

/* Loads the initial state of all E environments ("reset"): replaces
 * EnvironmentGenerator.generate (generator/environment_generator.py:52-106)
 * object construction, Anthill.__init__ area rasterisation (anthill.py:28-33),
 * RLApi.register_ants (RL_api.py:57-66) and Reward.setup (rewards/reward.py:12-19,
 * reward_custom.py:13-15,33-35,65-77).  timestep := 1 (environment.py:27). */
int antsrl_reset(AntsHandle *h, const AntsInit *init, void *stream);

/* Episode "reset" on the device: draws what EnvironmentGenerator.generate
 * draws (generator/environment_generator.py:52-106) — anthill in the central half, walls cleared on
 * the anthill, food discs zeroed on walls, rocks in the generator's band, ants in a disc of 0.8 r
 * around the anthill — and loads it exactly like antsrl_reset.  gen->rng_kind picks the random source:
 *   ANTSRL_RNG_COUNTER    a counter-based generator keyed on (episode_seed, global env id, item): the reference's
 *                         distributions, NOT its maps (the oracle's oracle_generate restates this generator);
 *   ANTSRL_RNG_REFERENCE  the reference's own MT19937 streams (Python's `random` and `np.random`, seeded like
 *                         environment_generator.py:53-55): env e equals EnvironmentGenerator(seed = episode_seed +
 *                         env_id_base + e)
 *                         — anthill, food discs, rocks, ants and per-ant seeds bit for bit (see ANTSRL_RNG_* above).
 * With gen->auto_reset the handle keeps `gen` and re-runs it after every finished episode: with episode_seed + 1,
 * + 2, ... (ANTSRL_RNG_COUNTER) or AntsCfg.n_envs_total seeds further each time (ANTSRL_RNG_REFERENCE: global env g of
 * episode k takes seed episode_seed + k * n_envs_total + g, whatever the sharding).  Two limits of that mode:
 * np.random.seed takes 32 bits, so (seed + env_id_base + E) * 5 must stay
 * below 2^32 — checked again at every auto-reset, which returns ANTSRL_E_INVALID instead of wrapping; and with
 * ANTSRL_WALLS_INPUT every episode re-uses the bitmaps of the first call (the reference calls walls_generator.generate
 * per episode: pass fresh bitmaps through antsrl_generate between episodes if the walls are to change). */
int antsrl_generate(AntsHandle *h, const AntsGen *gen, uint64_t episode_seed, void *stream);

/* RLApi.step (environment/RL_api.py:168-204): mandibles/food exchange, pheromone
 * activation, rotate, forward move, observation, reward, done.
 *   rotation  int8 [E][N] in {-1,0,1} or NULL (= leave theta unchanged, RL_api.py:190)
 *   phero     int8 [E][N] in {0,1,2}  or NULL (= leave activation, RL_api.py:187)
 *   obs         float [E][N][P][P][K]   perception  (may be NULL: skip the write — rewards, agent_state and, with
 *                                       antsrl_set_inloop_policy, the next actions are produced all the same: the
 *                                       act-only rollout of collect_agent_memory.py:189-199 with training=False)
 *   agent_state float [E][N][2]         [holding, seed], RL_api.py:160-162
 *   reward      float [E][N]            Reward.step, rewards/reward.py:38
 *   done        uint8 [E]               RL_api.py:200                         */
int antsrl_step(AntsHandle *h, const int8_t *rotation, const int8_t *phero, float *obs,
                float *agent_state, float *reward, uint8_t *done, void *stream);

/* RLApi.observation (environment/RL_api.py:96-165) on the current state, including
 * its reward side effects (reward.observation, RL_api.py:164).  reward may be NULL. */
int antsrl_observe(AntsHandle *h, float *obs, float *agent_state, float *reward, void *stream);

/* Environment.update (environment/environment.py:42-47): timestep += 1, then
 * Walls (walls.py:22-30), CircleObstacles (circle_obstacles.py:32-58), Pheromone
 * (pheromone.py:43-45), Ants (ants.py:123-130), Anthill (anthill.py:41-46).
 *   wall_jitter  double [E][N] or NULL.  When given, entry k of env e is the k-th
 *   value np.random.random(k) would have returned in Walls.update (walls.py:28):
 *   the k-th colliding ant, in ant-index order, consumes it.  NULL = built-in
 *   counter-based generator keyed on (AntsCfg.rng_seed, AntsCfg.env_id_base + e, timestep, ant).
 * DEFERRED UPDATE.  With wall_jitter == NULL on the cell-meta path (<= 1024 ants, ANTSRL_Q_DEFERRED_UPDATE; scaled
 * pheromone units or an explicit sweep alike) the call does the update's bookkeeping (and enqueues the pheromone sweep, if
 * there is one) and returns without enqueuing the update's kernel: the
 * next antsrl_step / antsrl_step_update runs it in the same launch as its move (k_update_move: the move re-reads
 * what the update has just written — one launch and most of the second kernel's HBM fetches saved).  Every other
 * entry point that reads or replaces the state (antsrl_observe, antsrl_read_state, antsrl_set_activation, a second
 * antsrl_update, antsrl_reset / antsrl_generate) enqueues or drops it first, on ITS stream argument: results are
 * the same as with an immediate launch, bit for bit; only the moment the kernel is enqueued moves.  Callers that
 * alternate streams between calls must order them as they already have to for the state itself.
 * In k_update_move the update hands the food word of each ant's cell to the move in a register under BOTH record layouts —
 * the interleaved 16-byte {p0, p1, food, META} records (ANTSRL_Q_INTERLEAVED) and the 8-byte {food, META} records, tiled or
 * row-major, beside separate pheromone buffers (explicit sweep, a filter with a radius) — so the move reads no food itself
 * and every food read of a step precedes every food write, as in the reference (ants.py:102-117).
 * WORKSPACE CONSISTENCY: while an update is deferred, the workspace still holds the pre-update state.  A caller that
 * copies or checkpoints the workspace bytes, records an event "after the update" or times the update on its own calls
 * antsrl_flush first. */
int antsrl_update(AntsHandle *h, const double *wall_jitter, void *stream);

/* Environment.update (environment/environment.py:42-47) ONE REFERENCE STEP AT A TIME, for callers whose own EnvObjects must
 * run BETWEEN the world's objects: the reference sorts every object of the environment by update_step() (stable) and calls
 * them in turn — Walls (-1), Food / CircleObstacles / Pheromone / RLApi (0), Ants (999), Anthill (1000); an object the
 * caller added with, say, update_step() == 500 runs after the rocks and the pheromone update and before the ants'.
 * antsrl_update_phase runs one of the four device steps and returns; the four calls in order are one antsrl_update, bit for
 * bit (same device functions, cut at launch boundaries; never deferred).  antsrl_read_state between two phases sees the
 * state as the reference's object would (positions already reverted off walls after WALLS, the decayed / diffused grid
 * after ROCKS_PHEROMONE, ...).  `wall_jitter` as for antsrl_update; only WALLS reads it.  Environment.timestep advances
 * with ANTHILL (the reference increments it before the first object: a binding that exposes `timestep` adds one while an
 * update is in progress).  While phases are outstanding every entry point that changes the state returns ANTSRL_E_INVALID. */
enum { ANTSRL_PHASE_WALLS = 0, ANTSRL_PHASE_ROCKS_PHEROMONE = 1, ANTSRL_PHASE_ANTS = 2, ANTSRL_PHASE_ANTHILL = 3 };
int antsrl_update_phase(AntsHandle *h, int phase, const double *wall_jitter, void *stream);

/* Enqueues a deferred update's kernel on `stream` now (no-op when none is pending): afterwards every kernel the
 * handle owes has been enqueued and, once `stream` has drained, the workspace holds the complete state.  No reference
 * counterpart (the reference updates eagerly; this is the price of k_update_move).  antsrl_destroy drops a pending
 * update with the handle: the workspace is the caller's, flush first if its content is still wanted. */
int antsrl_flush(AntsHandle *h, void *stream);

/* CHECKPOINT, RESTORE, FORK (no reference counterpart: the reference's state is a handful of numpy arrays that
 * copy.deepcopy handles).  A batch's state lies in two places: the workspace, whose carve depends on how the handle was
 * made (one block or two, placed anywhere), and the handle's host fields.  A checkpoint is a DEVICE BLOCK and a HOST BLOB.
 *
 * The device block holds every array of antsrl_workspace_map except pol_pack, in carve order, each stored whole
 * ([E][bytes_per_env]: every array of the carve is environment-major) and rounded up to 256 bytes.  It does not depend on
 * `split` or on where the workspace lies: a block saved from an antsrl_create handle loads into an antsrl_create2 handle of
 * the same AntsCfg and the other way round.  pol_pack is the caller's policy (antsrl_set_inloop_policy), not state: the
 * caller installs it again.  antsrl_checkpoint_map (host only, no handle) reports the block's arrays as
 * antsrl_workspace_map does the workspace's (min(*count, cap) entries written, any output pointer may be NULL) and the two
 * sizes: device_bytes, the block's (the end of its last array), and host_bytes, the blob's.
 *
 * The host blob is a versioned plain struct of host_bytes bytes, opaque to the caller: a magic, a format version, its own
 * size, the saving handle's whole AntsCfg, and every field of the handle that an entry point changes after antsrl_create
 * and that belongs to the episode — the current pheromone buffer, the steps since the last update, whether the next update
 * collects over the whole grid, the episode's seed and the kept generator (antsrl_generate), Environment.timestep's host
 * mirror, the scaled units' sweep count (the decay factors are recomputed from it), the explored summary's cadence and
 * whether it is consumed, the explored stamps' sequence number, a pending wall clear, the deposit strength
 * (antsrl_set_activation).  AntsGen.walls_input is a caller's pointer and is stored as NULL: a generator of kind
 * ANTSRL_WALLS_INPUT is NOT carried — the loading handle comes back without a kept generator (no auto-reset) until
 * antsrl_generate gives it one.  What belongs to the loading handle is not in the blob and stays as the handle has it: the
 * observation format and row stride, the perceive path, the in-loop policy, the timing events.  The explored summary is
 * consumed after a load when the checkpoint's was and the loading handle keeps one (ANTSRL_Q_EXPLORED_SUMMARY).
 *
 * antsrl_checkpoint_save: enqueues a deferred update first (the block holds the state behind it), then ONE copy kernel on
 * `stream`; the blob is written before the call returns, the block is complete once `stream` has drained.  device_block:
 * device memory of device_bytes bytes, 16-byte aligned, outside the workspace.
 * antsrl_checkpoint_load: the reverse, into a handle that holds an episode (antsrl_reset / antsrl_generate has been called;
 * whatever it held is replaced).  Refused with ANTSRL_E_INVALID, before anything is enqueued, when the blob's magic, version
 * or size is not this library's or its AntsCfg differs from the handle's in any byte (the message names the first field
 * that differs).  From a load on, every entry point continues bit for bit as the saving handle did from the save on.
 * The caller-owned outputs (obs, agent_state, reward, done) are the caller's to keep beside the checkpoint.
 *
 * antsrl_fork_envs: environment src[i] is copied over environment dst[i], i = 0 .. n - 1, inside the workspace (`src` and
 * `dst` are HOST arrays).  n >= 1, every index in [0, n_envs), the dst entries distinct, no dst entry among the src entries;
 * a src entry may repeat (one source fans out).  The pairs travel as kernel arguments: one launch per 640 pairs.  The
 * handle's host fields are shared by all its environments (they step in lockstep) and do not change.  A destination keeps
 * its own GLOBAL ENVIRONMENT ID (AntsCfg.env_id_base + index): with the library's own wall jitter (antsrl_update with
 * wall_jitter == NULL) its jitter stream is its own from the fork on, so a branch diverges from its source as soon as one
 * of its ants runs into a wall, even under equal actions; with explicit wall_jitter rows equal to the source's — or on a
 * map without walls — it repeats the source exactly.
 *
 * All three refuse a handle without an episode and one between two phases of antsrl_update_phase. */
typedef struct AntsCkptArray {
    char name[24];
    uint64_t offset, bytes_per_env;
} AntsCkptArray;
int antsrl_checkpoint_map(const AntsCfg *cfg, AntsCkptArray *entries, int32_t cap, int32_t *count, size_t *device_bytes,
                          size_t *host_bytes);
int antsrl_checkpoint_save(AntsHandle *h, void *device_block, void *host_blob, void *stream);
int antsrl_checkpoint_load(AntsHandle *h, const void *device_block, const void *host_blob, void *stream);
int antsrl_fork_envs(AntsHandle *h, const int32_t *src, const int32_t *dst, int32_t n, void *stream);

/* main.py:98 followed by main.py:131 — one full simulation step. */
int antsrl_step_update(AntsHandle *h, const int8_t *rotation, const int8_t *phero,
                       const double *wall_jitter, float *obs, float *agent_state, float *reward,
                       uint8_t *done, void *stream);

/* Measurement hook (no reference counterpart; the reference only keeps a wall-clock EMA,
 * main.py:93,132-136).  events = ANTSRL_TIMING_EVENTS caller-created hipEvent_t, or NULL to disable.
 * While set, the NEXT antsrl_step_update records them on its stream: [0] before the pheromone sweep,
 * [1] after it, [2] after the per-ant action kernel (k_move; equal to [1] where one kernel does both),
 * [3] after the perception kernel (k_perceive / k_act), [4] after the update kernel; the hook then
 * clears itself.  With a deferred update (antsrl_update) [1]..[2] brackets k_update_move — the PREVIOUS step's
 * update and this step's move — and [3]..[4] is empty under scaled units; under an explicit sweep the step's sweep
 * follows its kernels then ([0]..[1] empty, [3]..[4] brackets the sweep: the deferred deposits land in its input). */
#define ANTSRL_TIMING_EVENTS 5
int antsrl_set_timing_events(AntsHandle *h, void *const *events);

/* What the handle resolved its configuration to (no reference counterpart; bench.py and the tests name the
 * kernels and byte models from it). */
enum {
    ANTSRL_Q_CELL_META = 0,        /* 1: k_move + k_perceive on the cell-meta layout, 0: k_act           */
    ANTSRL_Q_SCALED_UNITS = 1,     /* 1: pheromone held in units of f0^S (no per-step sweep)              */
    ANTSRL_Q_INTERLEAVED = 2,      /* 1: {p0, p1, food, meta} 16-byte cell records                        */
    ANTSRL_Q_FILTER_SEPARABLE = 3, /* 1: DIFFUSE_FILTER detected as rank-1 (separable stencil march)      */
    ANTSRL_Q_PERCEIVE_RUN = 4,     /* ants per wave of k_perceive (0 without the cell-meta path)          */
    ANTSRL_Q_TIMESTEP = 5,         /* Environment.timestep (environment.py:27,45) as the host mirrors it: every env of a
                                      handle steps in lockstep, so no device read is needed                */
    ANTSRL_Q_DEFERRED_UPDATE = 6,  /* 1: antsrl_update(NULL jitter) is deferred into the next step (k_update_move) */
    ANTSRL_Q_PERCEIVE_FAST = 7,    /* 1: k_perceive runs its fast path (power-of-two grid, interleaved records in 2 x 4-cell
                                      blocks, a perception mask) and antsrl_set_perceive_path has not pinned the generic one */
    ANTSRL_Q_EXPLORED_SUMMARY = 8, /* 1: the handle, as it is set up now, keeps the explored summary and its k_perceive consumes
                                      it (see antsrl_set_perceive_path): the fast path with the rock channel perceived and no
                                      in-loop policy, a mask with masked cells, a reward that counts explored cells, a grid
                                      of at least 8 x 8 cells                                                    */
    ANTSRL_Q_COUNT_
};
int antsrl_query(const AntsHandle *h, int what, long long *value);

/* Measurement helper (no reference counterpart): a plain device-to-device copy of `bytes` bytes (multiple of
 * 16, both pointers 16-byte aligned) with 16 bytes per lane, enqueued on `stream` — bench.py times it for the
 * box's achievable read + write bandwidth next to the 8 TB/s specification. */
int antsrl_bench_copy(void *dst, const void *src, size_t bytes, void *stream);

/* Device memory for the step's big buffers — the workspace and the observation tensor — (no reference counterpart; the
 * step entry points never allocate: this is an allocator the CALLER may use for the buffers it owns).  The memory is one
 * virtual range backed by physical pieces of at most ANTSRL_MEM_PIECE_BYTES (hipMemCreate / hipMemMap).  On MI355X the
 * physical layout of these two buffers is worth 15 % of the observation kernel: when both lie in physically contiguous
 * ranges of 128 MiB or more (what hipMalloc hands a fresh process) the observation write stream and the cell-record
 * gathers alias on the memory channels; with either buffer in pieces of at most 32 MiB they do not — k_perceive 0.167 ms
 * against 0.197 ms at 1024 envs x 512 ants, on every allocation (profiles/history/r04/placement_probe4*.txt).  The pointer is
 * aligned to the device's allocation granularity (2 MiB); contents are undefined; free with antsrl_mem_free (never hipFree).
 * antsrl_mem_free waits for the block's device and PARKS the block, still mapped, in a per-device pool; antsrl_mem_alloc hands
 * a parked block of the same device and (piece-rounded) size back before it maps anything new.  Nothing is unmapped while
 * the program runs, so no address is ever translated to other memory than it was first mapped to (a range that is unmapped,
 * freed and reserved again can meet stale GPU translations on ROCm 7.2: antsrl_mem.hip) and the reserved address space is
 * bounded by the blocks that were alive at once.  antsrl_mem_trim returns the parked blocks' physical memory to the device
 * (their ranges are retired, never reused); antsrl_mem_stats reports bytes handed out / parked / reserved / retired (any
 * pointer may be NULL).  Returns ANTSRL_E_NOMEM when the device cannot supply the pieces, ANTSRL_E_DEVICE when the runtime
 * lacks the virtual-memory API. */
#define ANTSRL_MEM_PIECE_BYTES ((size_t)16 << 20)
int antsrl_mem_alloc(size_t bytes, int device, void **ptr);
int antsrl_mem_free(void *ptr);
int antsrl_mem_trim(void);
int antsrl_mem_stats(size_t *live_bytes, size_t *pooled_bytes, size_t *reserved_va_bytes, size_t *retired_va_bytes);

/* Observation tensor format (no reference counterpart: the reference's perception is float64 numpy,
 * cast to float32 by torch.Tensor(state) in the agents, collect_agent_memory.py:194).
 * ANTSRL_OBS_F32 (default): `obs` arguments are float [E][N][P][P][K].
 * ANTSRL_OBS_BF16: `obs` arguments point to bfloat16 (uint16_t) buffers of the same shape holding the
 * same values rounded to nearest even — half the bytes written per step, and what the bf16 policy
 * (antsrl_policy_mlp*) rounds its input to anyway.  Supported for 2 pheromone channels, the
 * generator's channel order and perceptions of at most 64 cells; otherwise the step returns
 * ANTSRL_E_UNSUPPORTED. */
#define ANTSRL_OBS_F32 0
#define ANTSRL_OBS_BF16 1
int antsrl_set_obs_format(AntsHandle *h, int format);

/* Observation row stride (no reference counterpart; opt-in, the default is the dense [E][N][P][P][K] tensor of
 * RL_api.py:122).  A row of P*P*K values is 1 372 bytes at the reference's 7x7x7 float32 perception: no row starts or ends
 * on a 128-byte line.  With stride_elems = the row rounded up to whole lines (float32 7x7x7: 352 elements = 1 408 bytes;
 * bfloat16: 384) the `obs` arguments point to [E][N][stride_elems] buffers (128-byte aligned): element k of ant a's
 * perception lies at a * stride_elems + k, the padding elements behind it are written as zeros, and every copy-out of
 * the observation kernel is whole lines of one wave's own.  A torch caller sees the reference's shape through a view:
 * buf.view(E, N, stride)[..., :P*P*K].view(E, N, P, P, K).  0 (or P*P*K) = dense.  Cell-meta path only
 * (ANTSRL_Q_CELL_META); not together with antsrl_set_inloop_policy; antsrl_set_obs_format resets it. */
int antsrl_set_obs_row_stride(AntsHandle *h, int32_t stride_elems);

/* Which k_perceive the handle launches (no reference counterpart; for tests and A/B runs).  The kernel has a fast path that
 * the library selects by itself where the configuration allows it (ANTSRL_Q_PERCEIVE_FAST) and a generic one for every
 * other grid and record layout; both compute the same bits.  ANTSRL_PERCEIVE_GENERIC pins the generic kernel,
 * ANTSRL_PERCEIVE_AUTO (the default) gives the choice back.
 * THE EXPLORED SUMMARY.  Where a reward counts explored cells, the records of the MASKED cells of a patch are gathered for
 * that count alone.  The fast path therefore keeps — where the rock channel is perceived and no in-loop policy is set: the
 * configurations in which it was measured to pay; everywhere else nothing is kept and nothing changes — one bit per tile of 8 x 8 cells, "every cell of this tile has been
 * explored", in the handle's workspace (the "explored_bits" array of antsrl_workspace_map, which nothing else uses on the
 * cell-meta path; bit (x / 8) * (H / 8) + y / 8, 32 bits per word) and skips those gathers for every ant whose patch lies
 * in tiles that have their bit: same results, fewer lines fetched.  The bits are cleared by antsrl_reset / antsrl_generate
 * (an auto-reset included) and set by a refresh the library enqueues behind the 256th, 512th and every 1024th observation
 * since; the kernel consults them from an episode's first refresh on (the library's own or antsrl_refresh_explored_summary).
 * ANTSRL_PERCEIVE_FAST_NOSKIP runs the fast kernel with the summary ignored and no refresh enqueued (A/B runs, tests);
 * ANTSRL_Q_EXPLORED_SUMMARY tells whether a handle keeps and consumes it. */
#define ANTSRL_PERCEIVE_AUTO 0
#define ANTSRL_PERCEIVE_GENERIC 1
#define ANTSRL_PERCEIVE_FAST_NOSKIP 2
int antsrl_set_perceive_path(AntsHandle *h, int path);

/* Enqueues a refresh of the explored summary now (antsrl_set_perceive_path), behind a pending deferred update as
 * antsrl_read_state does: every tile whose cells are all explored at that point gets its bit.  Returns ANTSRL_OK and does
 * nothing where the handle keeps no summary (ANTSRL_Q_EXPLORED_SUMMARY == 0). */
int antsrl_refresh_explored_summary(AntsHandle *h, void *stream);

/* Ants.activate_all_pheromones (environment/ants.py:86-87).  act: float [E][N][C].
 * new_deposit_strength > 0 also changes AntsCfg.deposit_strength (the dtype switch
 * of SURVEY.md §8(a) A4); pass 0 to keep it. */
int antsrl_set_activation(AntsHandle *h, const float *act, double new_deposit_strength,
                          void *stream);

/* In-loop policy inference (BASELINE config 5): the reference's linear DQN nets
 * (agents/explore_agent_pytorch.py:24-45, agents/collect_agent.py:24-51) evaluated on the
 * observation tensor without leaving the device, bf16 operands / fp32 accumulation (MFMA):
 *     out = layer1(cat[obs.view(M, F), agent_state.view(M, 2)])   layer1: w1 float [32][F+2], b1 [32]
 *     rotation  = argmax(layer2(out)) - 1                         layer2: w2 float [3][32],  b2 [3]
 *     pheromone = argmax(layer3(out))      (skipped if w3 NULL)   layer3: w3 float [3][32],  b3 [3]
 * Weights are PyTorch nn.Linear layouts, device pointers.  M = number of ants (E*N), F = P*P*K.
 * rotation/pheromone: int8 [M], directly usable as antsrl_step's actions.  logits (float [M][6],
 * nullable) receives the six head outputs.  `h` may be NULL; a handle set to ANTSRL_OBS_BF16
 * (antsrl_set_obs_format) makes `obs` a bfloat16 buffer of the same shape. */
int antsrl_policy_mlp(AntsHandle *h, const float *obs, const float *agent_state, int64_t n_ants, int32_t n_features,
                      const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                      const float *b3, int8_t *rotation, int8_t *pheromone, float *logits, void *stream);

/* The same network evaluated INSIDE the observation kernel (no reference counterpart; BASELINE config 5's loop:
 * action = agent.get_action(obs) of main.py:96 for the NEXT step, computed where the rows are produced).  While set,
 * every antsrl_step / antsrl_step_update / antsrl_observe — with an observation buffer or with obs == NULL — also stores
 *   rotation_next int8 [E][N] = argmax(layer2(out)) - 1     pheromone_next int8 [E][N] = argmax(layer3(out)) (or NULL)
 * for the rows it has just produced — the values antsrl_policy_mlp returns for that observation tensor, bit for bit
 * (same bf16 fragments, same order of MFMAs and additions) without re-reading it from HBM; with obs == NULL the rows
 * never leave the workgroup's LDS (no observation traffic at all).  Needs the cell-meta
 * path with bfloat16 observations (ANTSRL_Q_CELL_META, antsrl_set_obs_format); ANTSRL_E_UNSUPPORTED otherwise.
 * The weights (device pointers, float32, row-major like nn.Linear: w1 [32][n_features + 2], w2 / w3 [3][32]) are
 * copied into the handle's workspace at the call; w1 == NULL switches the in-loop policy off. */
int antsrl_set_inloop_policy(AntsHandle *h, int32_t n_features, const float *w1, const float *b1, const float *w2,
                             const float *b2, const float *w3, const float *b3, int8_t *rotation_next,
                             int8_t *pheromone_next, void *stream);

/* Recurrent memory agent net (no kernel counterpart in the reference; replaces the non-epsilon branch of
 * CollectAgentMemory.get_action, agents/collect_agent_memory.py:189-208, which evaluates CollectModelMemory.forward,
 * :57-78, on the host).  Per ant, x = cat[obs.view(F), agent_state(agent_dim), old_memory(mem_size)], D = F + agent_dim
 * + mem_size:
 *     g = L4(relu(L3(relu(L2(relu(L1(x))))))) + x            layer1 h2 x D, layer2 h3 x h2, layer3 h1 x h3, layer4 D x h1
 *     q_rot = R3(R2(R1(g)))   q_ph = P2(P1(g))   m = M2(M1(g))    (no activations; widths as in the reference's class)
 *     new_memory = tanh(M3(m)) * s + old_memory * (1 - s),  s = sigmoid(Fg(m))
 *     rotation = argmax(q_rot) - n_rot / 2,  pheromone = argmax(q_ph)   (first maximum on ties)
 * The reference's class has h1 = 2^(1+power), h2 = 2^(2+power), h3 = 2^(3+power) (power 5 in its code, 4 in its shipped
 * checkpoints) and agent_dim = 2.  Precision: bf16 MFMA operands (weights rounded once, every layer input rounded at the
 * MFMA), fp32 accumulation, fp32 biases / ReLU / residual (with the fp32 x) / tanh / sigmoid / blend; the carried memory
 * is read and written as fp32 and never rounded.
 * Supported: n_features >= 1, 1 <= agent_dim <= 32, 1 <= mem_size <= 32, D <= 1024, h1, h2, h3 multiples of 32 and
 * <= 256, 1 <= n_rot, n_ph <= 32; ANTSRL_E_UNSUPPORTED for positive values outside that, ANTSRL_E_INVALID for
 * values < 1 and missing pointers.  Validation happens before any HIP call. */
typedef struct AntsMemNetShape {
    int32_t n_features, agent_dim, mem_size, h1, h2, h3, n_rot, n_ph;
} AntsMemNetShape;

/* Size of the packed weights (host only; no HIP call).  With Dp = D rounded up to 32 and
 * frag(i, o) = 1024 * (i / 16) * (o / 32) bytes (bf16 MFMA fragments), bias(o) = 4 * o, each block rounded up to 256:
 *   the sum over the twelve packed layers (in, out) = (Dp, h2) (h2, h3) (h3, h1) (h1, Dp) (Dp, h2) (h2, h3) (h3, 32)
 *   (Dp, h1) (h1, 32) (Dp, h2) (h2, h2) (h2, 64) of round256(frag(in, out)) + round256(bias(out)).
 * 567 808 bytes at F = 294, power 5, mem_size 20; 236 032 at power 4, mem_size 10. */
int antsrl_memnet_packed_bytes(const AntsMemNetShape *s, size_t *bytes);

/* Converts the weights once into the kernel's private packed layout (one small kernel on `stream`).  params: host array
 * of the 26 device pointers of CollectModelMemory.state_dict() in its order (float32, nn.Linear layouts): layer1..4,
 * rotation_layer1..3, pheromone_layer1..2, memory_layer1..3, forget_layer, each .weight then .bias.  packed: device
 * buffer of antsrl_memnet_packed_bytes bytes, 256-byte aligned. */
int antsrl_memnet_pack(const AntsMemNetShape *s, const float *const *params, void *packed, void *stream);

/* The forward pass for n_ants ants (CollectAgentMemory.get_action's target_model call and torch.max, :194-200).
 * obs: [n_ants][F], float32 (ANTSRL_OBS_F32) or bfloat16 (ANTSRL_OBS_BF16); agent_state float [n_ants][agent_dim];
 * mem_in float [n_ants][mem_size] (the old memory, the tail of the reference's agent state, :57); mem_out float
 * [n_ants][mem_size], may equal mem_in (each ant reads its own row before writing it: in place is bit-identical);
 * rotation int8 [n_ants]; pheromone int8 [n_ants] or NULL; q_out float [n_ants][n_rot + n_ph] (rotation head then
 * pheromone head) or NULL. */
int antsrl_policy_memory(const AntsMemNetShape *s, const void *packed, const void *obs, int obs_format,
                         const float *agent_state, const float *mem_in, int64_t n_ants, float *mem_out, int8_t *rotation,
                         int8_t *pheromone, float *q_out, void *stream);

/* Precision of the memory agent net's forward (the _ex entries below; the entries above are ANTSRL_MEMNET_BF16).
 * ANTSRL_MEMNET_FP32: every MFMA operand is fp32 (weights, x, the hidden values, g, the head intermediates) and nothing
 * is rounded to bf16; accumulation and the epilogues are fp32 as above (v_mfma_f32_32x32x2_f32: each product is a
 * k-ordered fmaf chain; two chains per output tile, added once).  bf16 observations are widened exactly.  Results equal
 * the reference's fp32 forward up to fp32 summation order, and an ant's outputs depend only on its own inputs. */
#define ANTSRL_MEMNET_BF16 0
#define ANTSRL_MEMNET_FP32 1

/* antsrl_memnet_packed_bytes for a precision.  ANTSRL_MEMNET_BF16: the same size.  ANTSRL_MEMNET_FP32: the same sum with
 * frag(i, o) = 1024 * (i / 8) * (o / 32) bytes (fp32 MFMA fragments, 4 bytes per weight):
 * 1 128 960 bytes at F = 294, power 5, mem_size 20; 467 456 at power 4, mem_size 10.
 * An unknown precision is ANTSRL_E_INVALID, before any other check. */
int antsrl_memnet_packed_bytes_ex(const AntsMemNetShape *s, int precision, size_t *bytes);

/* antsrl_memnet_pack into the layout of `precision` (packed: antsrl_memnet_packed_bytes_ex bytes, 256-byte aligned). */
int antsrl_memnet_pack_ex(const AntsMemNetShape *s, int precision, const float *const *params, void *packed, void *stream);

/* antsrl_policy_memory with weights packed by antsrl_memnet_pack_ex in the same `precision`; every other argument and
 * rule as there. */
int antsrl_policy_memory_ex(const AntsMemNetShape *s, int precision, const void *packed, const void *obs, int obs_format,
                            const float *agent_state, const float *mem_in, int64_t n_ants, float *mem_out,
                            int8_t *rotation, int8_t *pheromone, float *q_out, void *stream);

/* antsrl_policy_memory_ex over a device-resident list of 32-ant tiles: the forward of part of a batch, decided on the
 * device (antsrl_agent_plan writes such a list; any other source will do).  With M = n_ants and T = ceil(M / 32), tile t
 * is ants [32 t, min(32 t + 32, M)).  tiles: int32 [T] on the device, of which entries [0, n) are read,
 * n = min(max(*n_live, 0), T); n_live: int32 [1] on the device; both required, 4-byte aligned.
 *   - Every ant of a listed tile gets in mem_out, rotation, pheromone and q_out exactly the bits antsrl_policy_memory_ex
 *     writes for it (an ant's outputs depend only on its own inputs, in both precisions).
 *   - Ants of tiles that are not listed are not written at all: their rows keep whatever the buffers held.
 *   - An entry outside [0, T) is skipped: it is compared before it is used and never becomes an address.
 *   - Entries need not be sorted.  They must be DISTINCT when mem_in == mem_out: a tile listed twice in place may read
 *     its own new memory as the old one.  (Out of place a duplicate writes the same bits twice.)
 * The host does not know n, so the launch covers T tiles: a workgroup whose first slot is at or beyond n leaves at once,
 * the spare waves of the last, partly filled workgroup walk its barriers and write nothing.  Every other argument, rule
 * and error code as antsrl_policy_memory_ex.  One launch, no host synchronisation. */
int antsrl_policy_memory_tiles(const AntsMemNetShape *s, int precision, const void *packed, const void *obs, int obs_format,
                               const float *agent_state, const float *mem_in, int64_t n_ants, float *mem_out,
                               int8_t *rotation, int8_t *pheromone, float *q_out, const int32_t *tiles,
                               const int32_t *n_live, void *stream);

/* On-device DQN training step of the memory agent net (replaces CollectAgentMemory.train, agents/collect_agent_memory.py:
 * 133-176: target forward, TD targets, MSE loss, backward, torch.optim.Adam).  Same shape and limits as
 * antsrl_policy_memory; observations are float32 (what the replay stores).  Two stages, so that a data-parallel caller
 * can reduce the gradient between them: antsrl_memtrain_grad (loss + flat gradient) and antsrl_memtrain_apply (Adam).
 * Only the 9 layers the loss reaches are trained (layer1-4, rotation_layer1-3, pheromone_layer1-2: the first 18 tensors
 * of the state_dict); the memory head is never changed and has no Adam state, as in the reference (its .grad is None).
 * Precision: bf16 MFMA operands (weights, layer inputs, output gradients), fp32 accumulation, fp32 biases / ReLU masks /
 * residual / TD target / dL/dq / bias gradients / loss / Adam, fp32 masters and moments.  No floating-point atomics:
 * bit-identical from run to run.  Every argument is validated before any HIP call; nothing synchronises the host.
 *
 * A net's STATE is one device buffer of state_bytes, 256-byte aligned:
 *   params  at 0: params_floats fp32, the 26 state_dict tensors in order, dense (weight [out][in], then bias [out])
 *   m       at m_off = round256(4 params_floats): trained_floats fp32 (Adam's exp_avg of the first 18 tensors, same order)
 *   v       at v_off = round256(m_off + 4 trained_floats): trained_floats fp32 (exp_avg_sq)
 *   packs   at round256(v_off + 4 trained_floats): bf16, per trained layer W [r32(out)][r32(in)] then W^T, zero padded
 *   state_bytes = round256(that + 2 x the pack elements), r32 = rounded up to 32.
 * With D = n_features + agent_dim + mem_size, the 13 layers (out, in) are (h2, D) (h3, h2) (h1, h3) (D, h1) (h2, D)
 * (h3, h2) (n_rot, h3) (h1, D) (n_ph, h1) | (h2, D) (h2, h2) (mem, h2) (mem, h2); params_floats = sum of out (in + 1)
 * over all 13, trained_floats over the first 9 (205 442 and 267 690 at F = 294, power 5, mem_size 20).
 * Workspace for B rows (Bp = r32(B)), in fp32 blocks each rounded up to 64 floats: 3 Bp r32(out) per trained layer
 * (target and model outputs, model output gradients), nchunk x sum over trained layers of r32(out) (r32(in) + 1)
 * (row-chunk gradient partials; nchunk = min(64, ceil(Bp / 256)) chunks of r32(ceil(Bp / nchunk)) rows, recounted as
 * ceil(Bp / chunk)), and ceil(Bp / 256) loss partials.  The blocks lie in this order, each [Bp][r32(out)] row-major:
 * the target net's nine layer outputs (state_dict order: layer1-4, rotation_layer1-3, pheromone_layer1-2), the model's
 * nine, the model's nine output gradients dh1 dh2 dh3 dg dr1 dr2 dqr dp1 dqp (dL/d of those outputs, the same order),
 * then the partials [nchunk][per layer: weight [r32(out)][r32(in)], then bias [r32(out)]], then the loss partials.
 * Padded columns of every block and padded rows of the output gradients and partials are written as 0; padded rows of
 * the layer outputs hold the net's output for x = 0.  1 <= B <= 2^24.  Outputs may be NULL. */
int antsrl_memtrain_sizes(const AntsMemNetShape *s, int64_t B, size_t *params_floats, size_t *trained_floats,
                          size_t *state_bytes, size_t *workspace_bytes);

/* state := the 26 device tensors params[] (CollectModelMemory.state_dict() order, float32), m = v = 0, packs rebuilt. */
int antsrl_memtrain_init(const AntsMemNetShape *s, const float *const *params, void *state, void *stream);

/* The 26 masters of `state` into the device tensors params[] (state_dict order). */
int antsrl_memtrain_unpack(const AntsMemNetShape *s, const void *state, float *const *params, void *stream);

/* target := model (:170-174): masters and packs of src_state into dst_state; Adam's m and v are not copied. */
int antsrl_memtrain_copy(const AntsMemNetShape *s, const void *src_state, void *dst_state, void *stream);

/* Stage 1 for B rows idx[0..B) (int64, values in [0, N): the caller guarantees it; NULL = rows 0..B-1) of the replay
 * arrays states float [N][n_features], agent_states float [N][agent_dim + mem_size], actions int64 [N][2] (rotation
 * index = rotation + n_rot / 2, pheromone index), rewards float [N], new_states, new_agent_states, dones bool [N]:
 *   y = r + discount * max(q_target(new)) * (1 - done) per head; loss = sum over the heads of mean over B x n_head of
 *   (q - target)^2 with target = q except y at the taken action.  An action index outside [0, n_head) contributes
 *   nothing (and is never used as an address).
 * Writes loss_out (float, on the device) and grads (float [trained_floats], the gradients of the 18 trained tensors in
 * the params layout).  `state` is the model, `target_state` the target net; workspace: antsrl_memtrain_sizes(B) bytes,
 * 256-byte aligned.  7 forward launches (both nets grouped per layer) + TD + 6 backward + weight gradient + reduction. */
int antsrl_memtrain_grad(const AntsMemNetShape *s, const void *state, const void *target_state, const float *states,
                         const float *agent_states, const int64_t *actions, const float *rewards, const float *new_states,
                         const float *new_agent_states, const uint8_t *dones, const int64_t *idx, int64_t B,
                         float discount, float *grads, float *loss_out, void *workspace, void *stream);

/* Stage 2: one torch.optim.Adam step (no weight decay, not amsgrad) over grads (float [trained_floats]) for optimizer
 * step `step` >= 1: m.lerp_(g, 1 - beta1); v = v beta2 + (1 - beta2) g^2; p -= lr / (1 - beta1^step) x
 * m / (sqrt(v) / sqrt(1 - beta2^step) + eps), the scalars computed in double on the host and rounded to float.  Then
 * the bf16 packs.  One launch. */
int antsrl_memtrain_apply(const AntsMemNetShape *s, void *state, const float *grads, int64_t step, double lr,
                          double beta1, double beta2, double eps, void *stream);

/* The memory agent's loop around the net and the training step (antsrl_memagent.hip; replaces the epsilon branch of
 * CollectAgentMemory.get_action, agents/collect_agent_memory.py:189-206, and update_replay_memory + ReplayMemory.extend,
 * :178-187 and agents/replay_memory.py:83-114).  Four entries on plain device pointers: every argument is validated
 * before any HIP call, nothing synchronises the host, and there are no atomics: results do not depend on scheduling.
 *
 * THE DRAW SPECIFICATION.  All randomness of these entries is counter-based, built from the mixer of the wall-jitter
 * stream (SplitMix64's finaliser; 64-bit unsigned arithmetic, wrapping):
 *     mix64(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *     draw(seed, tag, env, step, item):
 *         k = mix64(seed + 0x9E3779B97F4A7C15 * (env + 1))
 *         k = mix64(k ^ (0xD1B54A32D192ED03 * (step + 1)))
 *         k = mix64(k + 0x9E3779B97F4A7C15 * (item + 1))        (up to here: the key of the wall-jitter stream)
 *         k = mix64(k ^ tag)                                     (the stream tag: a fourth round the jitter stream lacks,
 *                                                                 so equal seeds never replay it, nor one another)
 *     u01(k)      = (double)(k >> 11) * 2^-53                     uniform in [0, 1), as the wall jitter makes it
 *     below(k, n) = ((k >> 32) * n) >> 32                         uniform integer in [0, n) by multiply-shift of the
 *                                                                 HIGH 32 bits; its bias is below n * 2^-32
 * `env` is always a GLOBAL environment id, env_id_base + e for environment e of the batch at hand, so a shard draws what
 * the full batch draws for its environments.  `step` is the caller's agent step counter, `seed` the caller's seed.
 * Streams (tag; env, item):
 *     ANTSRL_DRAW_EXPLORE    (env_id_base + e, 0):  does environment e explore this step
 *     ANTSRL_DRAW_ROTATION   (env_id_base + e, a):  the random rotation of ant a of environment e
 *     ANTSRL_DRAW_PHEROMONE  (env_id_base + e, a):  its random pheromone
 *     ANTSRL_DRAW_SAMPLE     (env_id_base,     j):  which transition replay entry j of the step records */
#define ANTSRL_DRAW_EXPLORE 0x45584C4FULL   /* "EXLO" */
#define ANTSRL_DRAW_ROTATION 0x524F5441ULL  /* "ROTA" */
#define ANTSRL_DRAW_PHEROMONE 0x50484552ULL /* "PHER" */
#define ANTSRL_DRAW_SAMPLE 0x53414D50ULL    /* "SAMP" */

/* Epsilon-greedy over n_envs x n_ants ants, in place behind antsrl_policy_memory(_ex) (get_action's else branch, :199-204).
 * One explore draw per environment and step (an environment is one reference colony; the reference draws once per colony
 * and step): environment e explores iff u01(draw(seed, ANTSRL_DRAW_EXPLORE, env_id_base + e, step, 0)) < epsilon, so
 * epsilon 0 never explores and epsilon 1 always does.  For every ant a of an exploring environment
 *     rotation  = below(draw(.., ANTSRL_DRAW_ROTATION, .., a), n_rot) - n_rot / 2     (np.random.randint(0, n_rot) - n_rot // 2)
 *     pheromone = below(draw(.., ANTSRL_DRAW_PHEROMONE, .., a), n_ph)
 *     mem_next[row of a] = mem_old[row of a]                                  ("we keep previous value", :204)
 * Every other environment's rotation, pheromone and mem_next stay bit for bit what the net wrote.
 * rotation, pheromone: int8 [n_envs][n_ants]; mem_old, mem_next: float [n_envs][n_ants][mem_size] (mem_old may equal
 * mem_next: nothing is copied then; a partial overlap is refused); explored: uint8 [n_envs] (1 = explored) or NULL.
 * 1 <= n_rot, n_ph, mem_size <= 32 (the net's limits), n_envs, n_ants >= 1, n_envs * n_ants < 2^31, env_id_base >= 0 with
 * env_id_base + n_envs < 2^31, 0 <= epsilon <= 1.  One launch. */
int antsrl_agent_select(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants, double epsilon,
                        int32_t n_rot, int32_t n_ph, int32_t mem_size, int8_t *rotation, int8_t *pheromone,
                        const float *mem_old, float *mem_next, uint8_t *explored, void *stream);

/* Which 32-ant tiles of the batch antsrl_agent_select will NOT overwrite entirely: the list antsrl_policy_memory_tiles
 * needs in front of it, so that the net is not evaluated for ants whose result select throws away.  With
 * M = n_envs * n_ants ants in the batch's flat order (ant i belongs to environment i / n_ants) and T = ceil(M / 32), tile t
 * is ants [32 t, min(32 t + 32, M)).  Tile t is LIVE iff at least one of its ants belongs to an environment that does not
 * explore at (seed, step) — "explores" exactly as in antsrl_agent_select: u01(draw(seed, ANTSRL_DRAW_EXPLORE,
 * env_id_base + e, step, 0)) < epsilon, the same double comparison.  So a tile that straddles an exploring and a
 * non-exploring environment (n_ants not a multiple of 32) is live, epsilon 0 lists all T tiles and epsilon 1 none.
 *   *n_live = the number of live tiles; tiles[0 .. *n_live) = their indices in ascending order;
 *   tiles[*n_live .. T) are unspecified (they are not written).
 * tiles: int32 [T], n_live: int32 [1], both on the device, required, 4-byte aligned.  n_envs, n_ants, env_id_base and
 * epsilon: the rules of antsrl_agent_select.  One launch of one workgroup (a prefix sum over the tiles' flags, no
 * atomics: the list does not depend on scheduling); no host synchronisation. */
int antsrl_agent_plan(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants, double epsilon,
                      int32_t *tiles, int32_t *n_live, void *stream);

/* One step's transitions into the seven rolling arrays of a replay memory (states float [max_len][n_features],
 * agent_states float [max_len][agent_dim + mem_size], actions int64 [max_len][2], rewards float [max_len], new_states,
 * new_agent_states, dones bool [max_len]), in two halves around the environment step, so that the observation the step
 * overwrites is never copied: antsrl_replay_record_pre before the step (behind antsrl_agent_select),
 * antsrl_replay_record_post after it, both with the SAME AntsRecordSpec.
 * Which ants: K of the M = n_envs * n_ants transitions, stratified.  Entry j (0 <= j < K) takes ant
 *     a_j = lo_j + min(floor(u_j * (hi_j - lo_j)), hi_j - lo_j - 1),  lo_j = floor(j * M / K),  hi_j = floor((j + 1) * M / K)
 *     u_j = u01(draw(seed, ANTSRL_DRAW_SAMPLE, env_id_base, step, j))       (a double product, rounded once, then floor;
 *                                                                            the min never binds: u_j <= 1 - 2^-53)
 * (ant a = e * n_ants + i, the batch's own order).  Both halves compute a_j from the same key, so no index array travels
 * between them; K == M is the identity, the reference's "every ant, in order".
 * Where: entry j goes to ring row (head + j) mod max_len; when K > max_len only the last max_len entries are written.
 * The caller then advances its head by K (mod max_len).
 *   pre:  states[row] = obs[a], agent_states[row] = agent_state[a] ++ memory[a],
 *         actions[row] = (rotation[a] + n_rot / 2, pheromone[a]; 1 when pheromone is NULL, replay_memory.py:100-103)
 *   post: rewards[row] = reward[a], new_states[row] = obs[a], new_agent_states[row] = agent_state[a] ++ memory[a],
 *         dones[row] = done[a / n_ants] != 0      (the environment's per-environment uint8)
 * obs: ant a's row of n_features values starts obs_pitch ELEMENTS behind ant a - 1's (0 = dense, n_features), float32
 * (ANTSRL_OBS_F32) or bfloat16 (ANTSRL_OBS_BF16, widened exactly: the ring is float32); agent_state float [M][agent_dim];
 * memory float [M][mem_size]; rotation, pheromone int8 [M]; reward float [M]; done uint8 [n_envs].
 * Limits: n_features >= 1, 1 <= agent_dim, mem_size, n_rot <= 32, n_features + agent_dim + mem_size <= 1024 (the net's),
 * n_envs, n_ants >= 1, M < 2^31, 1 <= K <= M, max_len >= 1, 0 <= head < max_len, obs_pitch 0 or >= n_features (and
 * below 2^24).  One launch each: one wave per entry; 16-byte loads and stores wherever a row's addresses allow them,
 * narrower ones where they do not (decided per row from the addresses themselves). */
typedef struct AntsRecordSpec {
    int32_t n_envs, n_ants, env_id_base;
    int32_t n_features, agent_dim, mem_size, n_rot;
    int32_t obs_format; /* ANTSRL_OBS_F32 / ANTSRL_OBS_BF16 */
    int32_t obs_pitch;  /* elements between two ants' rows; 0 = n_features */
    int32_t reserved;   /* 0 */
    int64_t K, head, max_len;
    uint64_t seed, step;
} AntsRecordSpec;

int antsrl_replay_record_pre(const AntsRecordSpec *r, const void *obs, const float *agent_state, const float *memory,
                             const int8_t *rotation, const int8_t *pheromone, float *states, float *agent_states,
                             int64_t *actions, void *stream);
int antsrl_replay_record_post(const AntsRecordSpec *r, const void *obs, const float *agent_state, const float *memory,
                              const float *reward, const uint8_t *done, float *rewards, float *new_states,
                              float *new_agent_states, uint8_t *dones, void *stream);

/* The loop without a memory, for the linear agent (CollectAgent, agents/collect_agent.py:150-177; its agent_states rows
 * are the 2 floats of agent_state).  antsrl_agent_select and AntsRecordSpec go on refusing mem_size == 0; these three
 * entries launch the SAME kernels without a memory operand, under the same draw specification and the same stream tags:
 * for equal (seed, step, env_id_base, n_envs, n_ants, epsilon, n_rot, n_ph) antsrl_agent_select_actions writes the
 * rotation, pheromone and explored bytes antsrl_agent_select writes, and for an AntsRecordSpec that differs in mem_size
 * alone (0 here) the _plain entries write the states, actions, rewards, new_states and dones rows the entries above
 * write; agent_states / new_agent_states are float [max_len][agent_dim], row = agent_state[a].  Every other rule (limits,
 * alignment, validation before any HIP call, one launch each, no atomics, no host synchronisation) is theirs. */
int antsrl_agent_select_actions(uint64_t seed, uint64_t step, int32_t env_id_base, int32_t n_envs, int32_t n_ants,
                                double epsilon, int32_t n_rot, int32_t n_ph, int8_t *rotation, int8_t *pheromone,
                                uint8_t *explored, void *stream);
int antsrl_replay_record_pre_plain(const AntsRecordSpec *r, const void *obs, const float *agent_state,
                                   const int8_t *rotation, const int8_t *pheromone, float *states, float *agent_states,
                                   int64_t *actions, void *stream);
int antsrl_replay_record_post_plain(const AntsRecordSpec *r, const void *obs, const float *agent_state, const float *reward,
                                    const uint8_t *done, float *rewards, float *new_states, float *new_agent_states,
                                    uint8_t *dones, void *stream);

/* The linear agent's training step: CollectAgent.train (agents/collect_agent.py:105-148) for the net antsrl_policy_mlp
 * evaluates (layer1 [32][F + 2], layer2 [3][32], layer3 [3][32]; F = n_features, n_features + 2 <= 1024).
 * What is trained: layer2 and layer3, 198 floats.  layer1 is frozen (CollectModel.__init__ clears its requires_grad; its
 * .grad stays None): it is only read, and has no Adam state.  Model and target net share ONE ExploreModel, so the target
 * net's rotation head is the live layer2 and only layer3 has a target copy.
 *   heads      float [198]: w2 [3][32] at 0, b2 [3] at 96, w3 [3][32] at 99, b3 [3] at 195 (the state_dict's order)
 *   target_l3  float [99]:  w3 [3][32] at 0, b3 [3] at 96
 *   adam_m, adam_v, grads: float [198], laid out like heads
 * Per minibatch row b (replay row i = idx[b], or b when idx is NULL; i is clamped to [0, n_rows)), with
 * x = states[i] ++ agent_states[i] and x' = new_states[i] ++ new_agent_states[i]:
 *     h  = layer1(x), h' = layer1(x')                     the sequence of antsrl_policy_mlp's flat form (k_policy_flat, the
 *                                                         form it takes whenever W1 and two 32-row images fit the LDS: every
 *                                                         F the reference's perception produces; its fallback for wider rows
 *                                                         feeds agent_state through the MFMA instead): x and w1 rounded to
 *                                                         bfloat16 (RNE), the F observation inputs accumulated in fp32 by
 *                                                         v_mfma_f32_32x32x16_bf16 in ascending 16-input steps, then
 *                                                         acc + (x[F] * w1[.][F] + x[F + 1] * w1[.][F + 1]) + b1 in fp32
 *     q_rot = layer2(h), q_ph = layer3(h)                 EVERYTHING FROM HERE ON IS fp32 on the fp32 masters (the acting
 *     q'_rot = layer2(h'), q'_ph = target_l3(h')          kernel rounds h and the head weights to bfloat16 for its second
 *     y_*  = rewards[i] + discount * max(q'_*) * !dones[i]  MFMA; the training forward does not: q - y feeds the gradient)
 *     d_rot = q_rot[actions[i][0]] - y_rot,  d_ph = q_ph[actions[i][1]] - y_ph        (action indices clamped to 0..2)
 *     loss  = sum_b (d_rot^2 + d_ph^2) / (3 B)            = MSE(q_rot, target_rot) + MSE(q_ph, target_ph), whose targets
 *     dL/dq = 2 d / (3 B) at the taken action, 0 elsewhere  are the no-grad q with the taken entry replaced by y
 *     grads = dL/dq^T h (weights), sum_b dL/dq (biases)
 * Sums over rows are taken in a fixed order (32 rows of a tile in row order per wave, a wave's tiles in order, waves in
 * order, workgroups in order) without atomics: equal inputs give equal bits.  Adam is torch.optim.Adam's single-tensor
 * arithmetic in fp32 per element (antsrl_memtrain_apply's), its step size and sqrt(1 - beta2^step) computed in double on
 * the host.  The target sync (target_l3 := heads[99 .. 198) when the caller's `done` counter says so) is one 396-byte
 * device copy of the caller's.
 * Launches: one for B <= 512 (one workgroup, whose 4 waves take up to 4 tiles each), else two (antsrl_lintrain_sizes
 * reports which).  workspace
 * (256-byte aligned, workspace_bytes) is needed for two launches only.  states / new_states float [n_rows][n_features],
 * agent_states / new_agent_states float [n_rows][2], actions int64 [n_rows][2], rewards float [n_rows], dones bool
 * [n_rows], idx int64 [B] or NULL, all on the device; loss: one device float.  1 <= B <= 2^24.
 *   _grad:  loss and grads; heads is not written.
 *   _apply: Adam on heads from grads; step >= 1 is Adam's step count.
 *   _step:  both in the same launches (grads may be NULL). */
int antsrl_lintrain_sizes(int32_t n_features, int64_t B, size_t *trained_floats, size_t *workspace_bytes, int32_t *launches);
int antsrl_lintrain_grad(int32_t n_features, const float *w1, const float *b1, const float *heads, const float *target_l3,
                         const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                         const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                         const int64_t *idx, int64_t B, float discount, float *grads, float *loss, void *workspace,
                         void *stream);
int antsrl_lintrain_apply(float *heads, float *adam_m, float *adam_v, const float *grads, int64_t step, double lr,
                          double beta1, double beta2, double eps, void *stream);
int antsrl_lintrain_step(int32_t n_features, const float *w1, const float *b1, float *heads, const float *target_l3,
                         float *adam_m, float *adam_v, const float *states, const float *agent_states,
                         const int64_t *actions, const float *rewards, const float *new_states,
                         const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B,
                         float discount, int64_t step, double lr, double beta1, double beta2, double eps, float *grads,
                         float *loss, void *workspace, void *stream);

/* The explore agent's training step: ExploreAgentPytorch.train (agents/explore_agent_pytorch.py:90-133) for ExploreModel
 * (:24-45; layer1 [32][F + 2], layer2 [3][32]; F = n_features, n_features + 2 <= 1024) — the net whose layer1 the linear
 * agent above freezes.  The reference class cannot run as written (its forward concatenates without dim=1, :43, and train
 * and get_action call the two-input model with one argument): this is what it means, CollectModel.forward's concat
 * (collect_agent.py:47-49) and the DQN step of the other agents.  BOTH layers are trained and the target net is a full
 * copy.  A net is ONE flat fp32 block of P = 32 (F + 2) + 32 + 96 + 3 floats in the state_dict's order:
 *   w1 [32][F + 2] at 0,  b1 [32] at 32 (F + 2),  w2 [3][32] at 32 (F + 2) + 32,  b2 [3] at 32 (F + 2) + 128
 * `model` and `target` are two such blocks; adam_m, adam_v and grads are float [P], laid out the same way.  target is only
 * read.  Per minibatch row b (replay row i = idx[b], or b when idx is NULL; i is clamped to [0, n_rows); a = actions[i][0]
 * clamped to 0..2), with x = states[i] ++ agent_states[i] and x' = new_states[i] ++ new_agent_states[i]:
 *     h  = layer1_model(x), h' = layer1_target(x')       the acting kernel's sequence, as for antsrl_lintrain_* above: x
 *                                                         and w1 rounded to bfloat16 (RNE), the F observation inputs
 *                                                         through v_mfma_f32_32x32x16_bf16 in ascending 16-input steps,
 *                                                         then acc + (x[F] w1[.][F] + x[F + 1] w1[.][F + 1]) + b1 in fp32
 *     q  = layer2_model(h), q' = layer2_target(h')        everything from here on is fp32 on the fp32 masters
 *     y  = rewards[i] + discount * max(q') * !dones[i],   d = q[a] - y
 *     loss  = sum_b d^2 / (3 B)                           MSELoss over [B, 3]: two of three entries are 0
 *     dq[b] = d * (2 / (3 B)) at a, 0 elsewhere;          g_w2 = dq^T h,  g_b2 = sum_b dq
 *     dh[b][j]   = dq[b][a] * w2[a][j]                    one fp32 product, never rounded to bfloat16
 *     g_w1[j][k] = sum_b dh[b][j] * bf16(x[b][k])         all F + 2 columns, agent_state's two included
 *     g_b1[j]    = sum_b dh[b][j]
 * Layer1's gradient is taken with the bfloat16-rounded x the forward used, against the fp32 master w1: a straight-through
 * gradient.  An Adam step at lr 1e-4 is about one bfloat16 ulp of a weight of size 0.05: steps accumulate in the fp32
 * master and reach the forward pass when the master crosses a rounding boundary.
 * Order of the sums over rows (no atomics; equal inputs give equal bits):
 *   g_w2, g_b2, loss: the 32 rows of a tile in row order from zero (product rounded, then added); a workgroup of the
 *       forward stage adds its four tiles' sums in tile order; the workgroups' sums are added in workgroup order.
 *   g_w1, g_b1: rows w, w + 16, w + 32, ... in ascending order by one fmaf per row from zero, for w = 0..15; then
 *       (((s0 + s1) + s2) + ...) + s15.
 * Adam is antsrl_lintrain_*'s (antsrl_adam.h) on all P floats, its step size and sqrt(1 - beta2^step) computed in double on
 * the host.  _grad followed by _apply gives the bits of _step.  The target sync is one device copy of the block, the
 * caller's.
 * Launches: two (the forward stage, one wave per 32 rows; the layer1 stage, one workgroup per 8 columns of the [32][F + 3]
 * product, which also runs Adam on its own columns).  workspace (256-byte aligned, workspace_bytes: the forward stage's
 * partial sums and dh [B][32]) is always needed.  Arrays as for antsrl_lintrain_*.  1 <= B <= 65536 (above:
 * ANTSRL_E_UNSUPPORTED).  Every argument is checked before anything is launched; no host synchronisation.
 *   _grad:  loss and grads; model is not written.
 *   _apply: Adam on model from grads; step >= 1 is Adam's step count.
 *   _step:  both in the same two launches (grads may be NULL). */
int antsrl_exptrain_sizes(int32_t n_features, int64_t B, size_t *trained_floats, size_t *workspace_bytes, int32_t *launches);
int antsrl_exptrain_grad(int32_t n_features, const float *model, const float *target, const float *states,
                         const float *agent_states, const int64_t *actions, const float *rewards, const float *new_states,
                         const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B,
                         float discount, float *grads, float *loss, void *workspace, void *stream);
int antsrl_exptrain_apply(int32_t n_features, float *model, float *adam_m, float *adam_v, const float *grads, int64_t step,
                          double lr, double beta1, double beta2, double eps, void *stream);
int antsrl_exptrain_step(int32_t n_features, float *model, const float *target, float *adam_m, float *adam_v,
                         const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                         const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                         const int64_t *idx, int64_t B, float discount, int64_t step, double lr, double beta1, double beta2,
                         double eps, float *grads, float *loss, void *workspace, void *stream);

/* The joint training step: CollectAgent.train (agents/collect_agent.py:105-148) with the freeze of layer1 lifted and
 * nothing else changed — the third stage of the linear agent's curriculum.  The reference's CollectModel clears
 * requires_grad on explore_model.layer1 but its Adam is built over all of model.parameters(): with requires_grad set
 * again, its own train() moves all six tensors, and that is what this is.  Model and target net share one ExploreModel,
 * so layer1 and layer2 are live in both nets and only layer3 has a target copy (a target copy of layer1 would be another
 * algorithm).  A net is ONE flat fp32 block of P = 32 (F + 2) + 32 + 198 floats in CollectModel.state_dict()'s order:
 *   w1 [32][F + 2] at 0,  b1 [32] at 32 (F + 2),  w2 [3][32] at 32 (F + 2) + 32,  b2 [3] at 32 (F + 2) + 128,
 *   w3 [3][32] at 32 (F + 2) + 131,  b3 [3] at 32 (F + 2) + 227
 * (the last four are antsrl_lintrain_*'s `heads` block); target_l3 is float [99] (w3 [3][32], b3 [3]) and only read;
 * adam_m, adam_v and grads are float [P], laid out as the net is, under ONE Adam step count.  Per minibatch row b (replay
 * row i = idx[b], or b when idx is NULL; i is clamped to [0, n_rows); a_rot, a_ph = actions[i][0], actions[i][1], each
 * clamped to 0..2), with x = states[i] ++ agent_states[i] and x' = new_states[i] ++ new_agent_states[i]:
 *     h = layer1(x), h' = layer1(x')                      BOTH through the same live w1 (one bfloat16 image of it, not
 *                                                         two), the acting kernel's sequence as for antsrl_lintrain_*: x
 *                                                         and w1 rounded to bfloat16 (RNE), the F observation inputs
 *                                                         through v_mfma_f32_32x32x16_bf16 in ascending 16-input steps
 *                                                         from a zero accumulator, then
 *                                                         acc + (x[F] w1[.][F] + x[F + 1] w1[.][F + 1]) + b1 in fp32
 *     q_rot = layer2(h), q_ph = layer3(h)                 everything from here on is fp32 on the fp32 masters
 *     y_rot = rewards[i] + discount * max(layer2(h')) * !dones[i]           the live layer2
 *     y_ph  = rewards[i] + discount * max(target_layer3(h')) * !dones[i]    (the TD targets carry no gradient)
 *     d_rot = q_rot[a_rot] - y_rot,  d_ph = q_ph[a_ph] - y_ph
 *     loss  = sum_b (d_rot^2 / (3 B) + d_ph^2 / (3 B))    MSELoss over [B, 3] per head, the two added
 *     dq_rot = d_rot * (2 / (3 B)) at a_rot, dq_ph = d_ph * (2 / (3 B)) at a_ph, 0 elsewhere
 *     g_w2 = dq_rot^T h, g_b2 = sum_b dq_rot, g_w3 = dq_ph^T h, g_b3 = sum_b dq_ph
 *     dh[b][j]   = dq_rot[b] * w2[a_rot][j] + dq_ph[b] * w3[a_ph][j]      two fp32 products and one add, each rounded
 *                                                                          on its own, in that order
 *     g_w1[j][k] = sum_b dh[b][j] * bf16(x[b][k])         all F + 2 columns, agent_state's two included
 *     g_b1[j]    = sum_b dh[b][j]
 * The gradient reaches layer1 only through the model's forward on x, from both heads; it is the straight-through gradient
 * of antsrl_exptrain_* (bfloat16 x against the fp32 master w1).
 * Order of the sums over rows (no atomics; equal inputs give equal bits):
 *   the 198 head gradients, loss: the 32 rows of a tile in row order from zero (product rounded, then added); a workgroup
 *       of the forward stage adds its four tiles' sums in tile order; the workgroups' sums are added in workgroup order.
 *   g_w1, g_b1: antsrl_exptrain_*'s, by the same device code: rows w, w + 16, w + 32, ... in ascending order by one fmaf
 *       per row from zero, for w = 0..15; then (((s0 + s1) + s2) + ...) + s15.
 * Adam is antsrl_lintrain_*'s (antsrl_adam.h) on all P floats.  _grad followed by _apply gives the bits of _step.  The
 * target sync is one device copy of layer3's 99 floats, the caller's.
 * Launches: two at every B (the forward stage, one wave per 32 rows, four waves per workgroup; the layer1 stage, one
 * workgroup per 8 columns of the [32][F + 3] product, and one more for the heads and the loss).  workspace (256-byte
 * aligned, workspace_bytes: the forward stage's partial sums, [workgroups][200] floats rounded up to 256 bytes, then
 * dh [B][32]; nothing follows row B - 1) is always needed.  Arrays as for antsrl_lintrain_*.  1 <= B <= 65536 (above:
 * ANTSRL_E_UNSUPPORTED).  Every argument is checked before anything is launched; no host synchronisation.
 *   _grad:  loss and grads; model is not written.
 *   _apply: Adam on model from grads; step >= 1 is Adam's step count.
 *   _step:  both in the same two launches (grads may be NULL). */
int antsrl_jointtrain_sizes(int32_t n_features, int64_t B, size_t *trained_floats, size_t *workspace_bytes, int32_t *launches);
int antsrl_jointtrain_grad(int32_t n_features, const float *model, const float *target_l3, const float *states,
                           const float *agent_states, const int64_t *actions, const float *rewards, const float *new_states,
                           const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B,
                           float discount, float *grads, float *loss, void *workspace, void *stream);
int antsrl_jointtrain_apply(int32_t n_features, float *model, float *adam_m, float *adam_v, const float *grads, int64_t step,
                            double lr, double beta1, double beta2, double eps, void *stream);
int antsrl_jointtrain_step(int32_t n_features, float *model, const float *target_l3, float *adam_m, float *adam_v,
                           const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                           const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                           const int64_t *idx, int64_t B, float discount, int64_t step, double lr, double beta1, double beta2,
                           double eps, float *grads, float *loss, void *workspace, void *stream);

/* The rework agent's net (no kernel counterpart in the reference; replaces the network branch of
 * CollectAgentRework.get_action, agents/collect_agent_rework.py:165-174, which evaluates target_model's
 * CollectModelRework.forward, :49-63, on the host).  Per ant, x = cat[obs.view(F), agent_state(2)], D = F + 2:
 *     general = layer4(layer3(layer2(layer1(x))))                        D -> g1 -> g2 -> g3 -> D
 *     q_rot   = rotation_layer4(rotation_layer3(rotation_layer2(rotation_layer1(general))))   D -> r1 -> r2 -> r3 -> n_rot
 *     q_ph    = pheromone_layer2(pheromone_layer1(general))              D -> p1 -> n_ph
 *     rotation = argmax(q_rot) - n_rot / 2,  pheromone = argmax(q_ph)    (first maximum on ties)
 * The reference's class has g1, g2, g3 = r1, r2, r3 = 64, 128, 32 and p1 = 32.  There is no activation anywhere, so both
 * heads are one affine map q = Wc x + bc, Wc [NQ][D], bc [NQ], NQ = n_rot + n_ph, the rotation rows first.  The layers are
 * multiplied out once per weight change (antsrl_rework_collapse: float64, rounded once to float32) and every step is NQ
 * fp32 dot products of length D per ant (antsrl_policy_rework).  There is one forward path: no layered mode, no precision
 * switch.  Against the float64 layered forward the collapsed form is no further off than torch's own fp32 layered forward.
 * Supported: n_features >= 1, agent_dim = 2, D <= 1024, every hidden width 1 .. 256, 1 <= n_rot, n_ph <= 8;
 * ANTSRL_E_UNSUPPORTED for positive values outside that, ANTSRL_E_INVALID for values < 1, missing or misaligned pointers,
 * an unknown obs_format and n_ants < 0.  Every check runs before any HIP call.  Each entry is one launch on `stream`: no
 * host synchronisation, no allocation. */
typedef struct AntsReworkShape {
    int32_t n_features, agent_dim,
            g1, g2, g3,      /* layer1..3 outputs: 64, 128, 32 in the reference's class */
            r1, r2, r3,      /* rotation_layer1..3 outputs: 64, 128, 32 */
            p1,              /* pheromone_layer1 output: 32 */
            n_rot, n_ph;
} AntsReworkShape;

/* Size of the collapsed buffer (host only; no HIP call): 4 * (NQ * D + NQ) bytes, Wc float [NQ][D] then bc float [NQ].
 * 7 128 bytes at F = 294, n_rot = n_ph = 3. */
int antsrl_rework_collapsed_bytes(const AntsReworkShape *s, size_t *bytes);

/* Multiplies the ten layers out (one small kernel, one workgroup per row of Wc).  params: host array of the 20 device
 * pointers of CollectModelRework.state_dict() in its order (float32, nn.Linear layouts [out][in], 4-byte aligned):
 * layer1..4, rotation_layer1..4, pheromone_layer1..2, each .weight then .bias.  collapsed: device buffer of
 * antsrl_rework_collapsed_bytes bytes, 4-byte aligned.
 * Row o of Wc starts as row o of its head's last layer (rotation_layer4 for o < n_rot, else pheromone_layer2 row
 * o - n_rot), v, with bc = that layer's bias; v is pushed down through rotation_layer3, 2, 1 (pheromone_layer1), then
 * layer4, 3, 2, 1.  A push through layer l (W_l [out][in], b_l [out]) is, in float64 with every product rounded before it
 * is added and the contracted index i ascending,
 *     bc <- ((bc + v[0] b_l[0]) + v[1] b_l[1]) + ...        v'[c] = ((0 + v[0] W_l[0][c]) + v[1] W_l[1][c]) + ...
 * and Wc[o][c] = (float)v[c], bc[o] = (float)bc after the last: one rounding each.  No atomics: equal weights give equal
 * bits in every launch.  Call it again whenever the weights change (the target net's: once per episode under the
 * reference's UPDATE_TARGET_EVERY = 1). */
int antsrl_rework_collapse(const AntsReworkShape *s, const float *const *params, void *collapsed, void *stream);

/* The forward pass and both argmaxes for n_ants ants (get_action's target_model call and torch.max, :170-174).
 * collapsed: what antsrl_rework_collapse wrote; obs: [n_ants][F], float32 (ANTSRL_OBS_F32) or bfloat16 (ANTSRL_OBS_BF16,
 * widened exactly), dense, 4-byte aligned; agent_state float [n_ants][2]; rotation int8 [n_ants] = argmax - n_rot / 2 and
 * pheromone int8 [n_ants], both required, directly usable as antsrl_step's actions; q_out float [n_ants][NQ] (rotation head
 * then pheromone head) or NULL.  n_ants == 0 succeeds and launches nothing; n_ants < 2^31.
 * Arithmetic is fp32 throughout.  Sixteen lanes share a row; with l the lane's place among them,
 *     a_l = 0;  for k = 4 l .. 4 l + 3, then 64 + 4 l .. , ... ascending:  a_l = fmaf(x[k], Wc[o][k], a_l)
 *     a = the a_l added pairwise: l with l ^ 1, then with l ^ 2, then with 7 - l inside its eight, then with 15 - l
 *     q[o] = a + bc[o]
 * so an ant's q and actions depend only on its own inputs and the collapsed buffer: not on n_ants, its place in the
 * batch, its neighbours or the grid, nor on the observation format when the values are equal; a launch repeated gives
 * the same bits.  No load touches a byte outside obs, agent_state and the collapsed buffer; nothing but rotation,
 * pheromone and q_out is written. */
int antsrl_policy_rework(const AntsReworkShape *s, const void *collapsed, const void *obs, int obs_format,
                         const float *agent_state, int64_t n_ants, int8_t *rotation, int8_t *pheromone, float *q_out,
                         void *stream);

/* antsrl_policy_rework and the epsilon-greedy select behind it (get_action's two branches, :165-174) in ONE launch, for
 * n_envs colonies of n_ants ants (rows in the batch's own order: ant a of colony e is row e * n_ants + a).  For equal
 * arguments it writes, bit for bit, the rotation, pheromone and explored bytes that
 *     antsrl_policy_rework(s, collapsed, obs, obs_format, agent_state, n_envs * n_ants, rotation, pheromone, ..)
 *     antsrl_agent_select_actions(seed, step, env_id_base, n_envs, n_ants, epsilon, s->n_rot, s->n_ph, rotation,
 *                                 pheromone, explored, ..)
 * write one after the other, under THE DRAW SPECIFICATION above and its stream tags as they are: colony e explores iff
 * u01(draw(seed, ANTSRL_DRAW_EXPLORE, env_id_base + e, step, 0)) < epsilon (the same double comparison), and its ant a
 * then takes below(draw(.., ANTSRL_DRAW_ROTATION, .., a), n_rot) - n_rot / 2 and below(draw(.., ANTSRL_DRAW_PHEROMONE,
 * .., a), n_ph).  What it saves is the forward pass of the exploring colonies: a run of eight consecutive rows that all
 * explore is neither loaded nor multiplied, so the observation and agent_state rows of an exploring colony need not hold
 * meaningful values (a run that mixes exploring and other rows is evaluated whole; what it computes for an exploring row
 * goes nowhere).  Rows of the other colonies get antsrl_policy_rework's arithmetic and bits.
 * explored: uint8 [n_envs] (1 = explored) or NULL; q_out: float [n_envs * n_ants][NQ] or NULL: the rows of the colonies that
 * do not explore get antsrl_policy_rework's q, the rows of the exploring ones are NOT written.
 * Rules: antsrl_policy_rework's (shape, pointers, alignment, obs_format) and antsrl_agent_select's (n_envs, n_ants >= 1,
 * n_envs * n_ants < 2^31, env_id_base >= 0 with env_id_base + n_envs < 2^31, 0 <= epsilon <= 1), all checked before any
 * HIP call.  One launch, no atomics, no host synchronisation, no allocation; each output byte has one writer and a
 * repeated launch gives the same bits.  No load touches a byte outside obs, agent_state and the collapsed buffer. */
int antsrl_policy_rework_select(const AntsReworkShape *s, const void *collapsed, const void *obs, int obs_format,
                                const float *agent_state, uint64_t seed, uint64_t step, int32_t env_id_base,
                                int32_t n_envs, int32_t n_ants, double epsilon, int8_t *rotation, int8_t *pheromone,
                                uint8_t *explored, float *q_out, void *stream);

/* The rework agent's training step: CollectAgentRework.train (agents/collect_agent_rework.py:110-152) for the net above,
 * all 20 tensors trained.  A net is ONE flat fp32 block of P floats (params_floats): the 20 tensors of the state_dict in its
 * order (layer1..4, rotation_layer1..4, pheromone_layer1..2, each .weight [out][in] then .bias), dense.  `model` is such a
 * block; adam_m, adam_v and grads are float [P], laid out the same way.  The TARGET net enters as its collapsed buffer
 * (target_collapsed: what antsrl_rework_collapse wrote for it, the acting policy's), which is only read.
 * Per minibatch row b (replay row i = idx[b], or b when idx is NULL; i is clamped to [0, n_rows); a_rot = actions[i][0]
 * clamped to [0, n_rot), a_ph = actions[i][1] to [0, n_ph)), x = states[i] ++ agent_states[i], x' the successor's:
 *     q  = Wc x + bc          the MODEL's collapsed form (float64 chain, rounded once: antsrl_rework_collapse's bits),
 *     q' = Wc' x' + bc'       the target's; both in fp32 in antsrl_policy_rework's order of sums
 *     per head (n outputs):   y = rewards[i] + discount * max(q'_head) * !dones[i],   d = q[a] - y,   g = d * (2 / (n B))
 *     loss = sum_b d_rot^2 / (n_rot B) + sum_b d_ph^2 / (n_ph B)        MSELoss of both heads; each scale applied once
 *     G [NQ][D] = sum_b (g_rot x at row a_rot, g_ph x at row n_rot + a_ph),   s [NQ] likewise without x       fp32
 * The net has no activation, so with M_l [NQ][out_l] the head rows pushed down to layer l's output (antsrl_rework_collapse's
 * v on its way; the unit rows at a head's last layer; zero in the other head's layers) and A_l [NQ][out_l] the pseudo-rows
 * pushed up, A_l = A_in(l) W_l^T + s (x) b_l with A of x being G (in(l): layer4 for rotation_layer1 and pheromone_layer1),
 *     dW_l = sum_k M_l[k] (x) A_in(l)[k],   db_l = sum_k M_l[k] s[k]
 * k over all NQ pseudo-rows for layer1..4, over the head's own for its layers.  Both chains and these sums are float64, every
 * product rounded before it is added, the contracted index (k here) ascending from zero, the bias term s[k] b_l[j] added
 * last; each gradient is rounded once to fp32.  No B x width activation is stored.
 * Order of the fp32 sums over rows (no atomics; equal inputs give equal bits whatever ran before): a workgroup of the batch
 * pass takes the rows 16 (w + i parts) .. + 15, i = 0, 1, ..., and adds them in ascending order from zero, the product g x
 * rounded first; the workgroups' partials are added in workgroup order from zero.
 * Launches: four (down chain, batch pass, up chain, gradient with Adam).  workspace (256-byte aligned, workspace_bytes) is
 * always needed; with NQ = n_rot + n_ph, out_l the outputs of layer l and every part rounded up to 256 bytes, in this order:
 *     collapsed  float  [NQ D + NQ]                 the model's Wc, bc
 *     M_l        double [NQ][out_l], l = 0..9
 *     partials   float  [parts][stride]             parts = min(ceil(B / 16), 256), stride = NQ D + NQ + 2 rounded up to 64:
 *                                                   G at 0, s at NQ D, sum d_rot^2 and sum d_ph^2 behind it
 *     G, s       float  [NQ D + NQ]
 *     A_l        double [NQ][out_l], l = 0..6 and 8
 * Adam is antsrl_lintrain_*'s (antsrl_adam.h) on all P floats.  _grad followed by _apply gives the bits of _step.  The target
 * sync is the caller's: a device copy of the block and one antsrl_rework_collapse.  Shapes: the net's supported range above;
 * 1 <= B <= 65536 (above: ANTSRL_E_UNSUPPORTED).  Arrays as for antsrl_lintrain_*.  Every argument is checked before
 * anything is launched; antsrl_reworktrain_sizes makes no HIP call; no host synchronisation.
 *   _grad:  loss and grads; model is not written.
 *   _apply: Adam on model from grads; step >= 1 is Adam's step count.
 *   _step:  both in the same four launches (grads may be NULL). */
int antsrl_reworktrain_sizes(const AntsReworkShape *s, int64_t B, size_t *params_floats, size_t *workspace_bytes,
                             int32_t *launches);
int antsrl_reworktrain_grad(const AntsReworkShape *s, const float *model, const float *target_collapsed, const float *states,
                            const float *agent_states, const int64_t *actions, const float *rewards, const float *new_states,
                            const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx,
                            int64_t B, float discount, float *grads, float *loss, void *workspace, void *stream);
int antsrl_reworktrain_apply(const AntsReworkShape *s, float *model, float *adam_m, float *adam_v, const float *grads,
                             int64_t step, double lr, double beta1, double beta2, double eps, void *stream);
int antsrl_reworktrain_step(const AntsReworkShape *s, float *model, const float *target_collapsed, float *adam_m,
                            float *adam_v, const float *states, const float *agent_states, const int64_t *actions,
                            const float *rewards, const float *new_states, const float *new_agent_states,
                            const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, float discount,
                            int64_t step, double lr, double beta1, double beta2, double eps, float *grads, float *loss,
                            void *workspace, void *stream);

/* The training monitor: what the reference's driver keeps around its step (main.py:66-152), resident on the device, so
 * that a training curve costs one launch per step and no host synchronisation.  Its state is ONE caller-allocated device
 * block (8-byte aligned, antsrl_monitor_sizes bytes) of float64 / int64 words, dense, in this order, for E = n_envs
 * environments of N = n_ants ants:
 *     episode_reward  double [E][N]                   main.py:89, one array per environment
 *     avg_loss        double                          main.py:59, :106-109: the running loss
 *     n_losses        int64                           losses seen so far; 0 is main.py's `avg_loss is None`
 *     last_loss       double                          the last loss seen
 *     reports         double [max_reports][E][3]      {total, min, max} of episode_reward[e][:] (main.py:115-120)
 *     episodes        double [max_episodes][3]        {grand_total, avg_loss, n_losses} (main.py:151-152), a row per episode
 * so bytes = 8 * (E N + 3 + 3 E max_reports + 3 max_episodes).  The means (main.py:116) are the caller's division: the
 * device divides nothing.
 *   _init:  zeroes the block (+0.0 and 0).
 *   _step:  ONE launch.  episode_reward[e][n] += (double)reward[e][n] (main.py:100; what numpy does for float64 +=
 *           float32).  With has_loss, the loss is *loss_dev when loss_dev is not NULL (the 0-d tensor a training step
 *           returns, read on the device) and loss_host otherwise (the host's 0 below min_replay, which the reference feeds
 *           into the average too): the first loss becomes avg_loss, a later one gives 0.99 * avg_loss + 0.01 * (double)loss
 *           with each product rounded before the add; n_losses += 1, last_loss = (double)loss.  With report_slot >= 0 the
 *           launch also writes reports[report_slot][e] from the updated episode_reward; report_slot = -1: no report, and
 *           then nothing is reduced.
 *   _end_episode:  ONE launch.  episodes[episode_slot] = {grand_total, avg_loss, (double)n_losses}, where grand_total is
 *           the sum over the environments of `total` in reports[last_report_slot], or 0 for last_report_slot = -1 (an
 *           episode without a report: main.py:90's mean_reward = 0, which goes stale between reports); then
 *           episode_reward = +0.0.  avg_loss, n_losses and last_loss carry over (main.py sets avg_loss before the episode
 *           loop).
 * THE ORDER OF THE SUMS (float64 adds, round to nearest even; no atomics: equal inputs give equal bits whatever ran
 * before).  One workgroup of 256 threads per environment: slot t starts at +0.0 and adds the ants t, t + 256, t + 512, ...
 * in ascending order; the 256 slots are folded with x[i] += x[i + s] for i < s, s = 128, 64, ..., 1; total = x[0].
 * grand_total folds the environments' totals by the same rule in one workgroup (slot t takes the environments t, t + 256,
 * ...).  min and max are order-free (a slot starts from its first ant, no infinity enters); a NaN reward is not ordered
 * and leaves them undefined.
 * Rules, all checked before any HIP call (ANTSRL_E_INVALID): state not NULL and 8-byte aligned; n_envs, n_ants >= 1 with
 * n_envs * n_ants < 2^31 - 256; max_reports, max_episodes >= 1; reward not NULL, reward and loss_dev 4-byte aligned;
 * report_slot and last_report_slot in [-1, max_reports), episode_slot in [0, max_episodes): a slot is never wrapped or
 * overwritten silently.  antsrl_monitor_sizes makes no HIP call; no entry allocates or synchronises the host. */
int antsrl_monitor_sizes(int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes, size_t *bytes);
int antsrl_monitor_init(void *state, int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes,
                        void *stream);
int antsrl_monitor_step(void *state, int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes,
                        const float *reward, const float *loss_dev, double loss_host, int has_loss, int report_slot,
                        void *stream);
int antsrl_monitor_end_episode(void *state, int32_t n_envs, int32_t n_ants, int32_t max_reports, int32_t max_episodes,
                               int episode_slot, int last_report_slot, void *stream);

/* The episode recorder: the replay viewer's snapshots (Environment.save_state, environment.py:36-40: the visualisation
 * copies main.py:138 keeps after every step of a visualised episode) of up to ANTSRL_RECORDER_MAX_ENVS chosen
 * environments, packed into a device-resident frame log with ONE launch per step and nothing read back.  The log is ONE
 * caller-allocated device block (16-byte aligned, `bytes` of antsrl_recorder_sizes); the caller copies it to the host at
 * the episode's end and decodes it (antsrl_amd/recorder.py).
 *
 * The block, for S = n_sel environments of N ants, R rocks, C pheromone channels and G = W * H cells.  Every section
 * starts 16-byte aligned: a section of n bytes takes a16(n) = n rounded up to 16, and the kernels write its padding as
 * zeros.  First the static part, static_bytes = S * (16 + 16 R + a16(G)); per selected environment, in the order of
 * env_indices:
 *     anthill_xyr   int32 [3], 4 bytes of zeros       Anthill.x, .y, .radius
 *     rock_rw       double [R][2]                      {radius, weight} per rock
 *     walls         uint8 [W][H]                       Walls.map (0 / 1)
 * then max_frames frames of frame_bytes each, frame f at static_bytes + f * frame_bytes; a frame holds the S
 * environments in the order of env_indices, frame_bytes = S * (32 + 16 R + a16(24 N) + a16(4 N) + 2 a16(N) +
 * (C + 1 + X) a16(G)) with X = 1 when the explored section is present; per environment:
 *     timestep      int32, 12 bytes of zeros           Environment.timestep
 *     anthill_food  double, 8 bytes of zeros           Anthill.food
 *     rock_centers  double [R][2]
 *     ants_xyt      double [N][3]                      Ants.ants
 *     holding       float  [N]
 *     mandibles     uint8  [N]
 *     reward_state  uint8  [N]
 *     phero         uint8  [C] planes of [W][H], each plane a16(G) bytes     pheromone.py:17
 *     food          uint8  [W][H]                      food.py:10
 *     explored      uint8  [W][H] (0 / 1)              the reward's explored_map: present only with with_heatmap != 0 on a
 *                                                      handle whose reward kind keeps one (ANTSRL_REWARD_EXPLORATION,
 *                                                      ANTSRL_REWARD_ALL); otherwise the section is absent, not zero
 * The values are what antsrl_read_state gives for ANTSRL_S_PHERO, _FOOD, _EXPLORED, _WALLS and the per-ant / per-env
 * selectors at the same moment, on every layout the handle can be in; phero and food are then cast to uint8.
 * THE CAST: (uint8_t)(int32_t)v, truncation toward zero, for 0 <= v < 256, which is numpy's astype(np.uint8) there; a
 * value of 256 or more SATURATES to 255 (a pheromone without max_val, a food pile above 255: numpy's result for those
 * is platform-defined).
 *   _sizes:  the three sizes (any of the pointers may be NULL); no HIP call.
 *   _begin:  ONE launch: the static part.  Call it after antsrl_reset / antsrl_generate and before the episode's first
 *            _frame; with AntsGen.auto_reset the walls, the anthill and the rocks change at the reset, so the caller
 *            calls _begin again at an episode boundary.
 *   _frame:  ONE launch: frame `frame` of the block, from the state as it stands.  A frame is the state AFTER
 *            Environment.update (where main.py:138 takes it): like antsrl_read_state, _begin and _frame first enqueue a
 *            deferred update on their stream argument (see antsrl_update), which therefore does not fuse with the next
 *            step's move.
 * env_indices is a HOST array of n_sel distinct indices in [0, n_envs); they travel to the kernel by value.  The same
 * n_sel, max_frames and with_heatmap go to every call on one block (they fix its layout).
 * Rules, all checked before any HIP call (ANTSRL_E_INVALID, the block untouched): block not NULL and 16-byte aligned;
 * 1 <= n_sel <= ANTSRL_RECORDER_MAX_ENVS; env_indices not NULL, every index in [0, n_envs), none repeated;
 * max_frames >= 1; frame in [0, max_frames): a frame is never wrapped; a handle that has been reset; no
 * Environment.update in progress (antsrl_update_phase).  No entry allocates or synchronises the host. */
#define ANTSRL_RECORDER_MAX_ENVS 8
int antsrl_recorder_sizes(const AntsHandle *h, int32_t n_sel, int32_t max_frames, int32_t with_heatmap,
                          size_t *static_bytes, size_t *frame_bytes, size_t *bytes);
int antsrl_recorder_begin(AntsHandle *h, void *block, const int32_t *env_indices, int32_t n_sel,
                          int32_t max_frames, int32_t with_heatmap, void *stream);
int antsrl_recorder_frame(AntsHandle *h, void *block, const int32_t *env_indices, int32_t n_sel,
                          int32_t max_frames, int32_t with_heatmap, int32_t frame, void *stream);

/* The colony statistics: what a training run reports of the task itself — the food a colony brought home (the number
 * the reference's viewer prints, FOOD IN ANTHILL, gui/visualize.py:247), the food left on the map and in the mandibles,
 * the explored cells, the pheromone on the map — as ONE row per call, reduced on the device in two launches, nothing
 * read back.  The block is caller-allocated device memory (8-byte aligned, `bytes` of antsrl_stats_sizes): max_rows rows
 * and then the scratch for the segments' partials.  A row is E = n_envs records of Q = 7 + 2 C dense 8-byte words, C =
 * n_phero; row r lies at r * row_bytes, environment e's record at word e * Q of it:
 *     word 0       int64    timestep[e]        ANTSRL_S_TIMESTEP
 *          1       double   anthill_food[e]    ANTSRL_S_ANTHILL_FOOD, copied, not summed
 *          2       double   food_left          the sum of (double)food[e][g] over the grid (ANTSRL_S_FOOD)
 *          3       int64    food_cells         cells with food > 0
 *          4       double   food_carried       the sum of (double)holding[e][n] (ANTSRL_S_HOLDING)
 *          5       int64    n_carrying         ants with holding > 0
 *          6       int64    explored_cells     cells with ANTSRL_S_EXPLORED != 0; -1 where the reward kind keeps no
 *                                              explored map (only ANTSRL_REWARD_EXPLORATION and ANTSRL_REWARD_ALL keep one)
 *          7 + 2c  double   phero_mass[c]      the sum of the materialised (double)phero[e][c][g] (ANTSRL_S_PHERO_C<c>:
 *                                              scaled units times g_now, zero below the threshold)
 *          8 + 2c  int64    phero_cells[c]     cells whose materialised value is > 0
 * Every value is what antsrl_read_state gives at the same moment, on every layout the handle can be in.
 * row_bytes = 8 E Q;  scratch_bytes = 8 E nseg (3 + 2 C) with nseg = ceil(G / 4096), G = W * H;  bytes = max_rows *
 * row_bytes + scratch_bytes.  The scratch is rewritten by every row and means nothing to the caller.
 * THE ORDER OF THE SUMS (float64 adds, round to nearest even; no atomics: equal state gives equal bits).  Cells: the
 * canonical cell ids g = x * H + y of an environment are cut into segments of 4096; one workgroup of 256 threads per
 * (segment, environment): slot t starts at +0.0 / 0 and takes the cells seg * 4096 + t + 256 k, k = 0, 1, ..., in
 * ascending order, skipping g >= G; the 256 slots are folded with x[i] += x[i + s] for i < s, s = 128, 64, ..., 1; x[0]
 * is the segment's partial, written to the scratch.  Second stage: one workgroup per environment: slot t takes the
 * partials of the segments t, t + 256, ... in ascending order, with the same fold; the same workgroup sums holding as
 * the training monitor sums rewards (slot t takes the ants t, t + 256, ..., the same fold) and copies timestep and
 * anthill_food.  The counts are int64 and exact; they take the same path.
 *   _sizes:  the three sizes (any of the pointers may be NULL); no HIP call.
 *   _row:    TWO launches: row `row` of the block, from the state as it stands.  Like antsrl_read_state and
 *            antsrl_recorder_frame it first enqueues a deferred update on its stream argument (see antsrl_update): a row
 *            is the state AFTER Environment.update, and the step behind a row does not fuse its update with the move.
 * The same max_rows goes to every call on one block (it fixes where the scratch lies).
 * Rules, all checked before any HIP call (ANTSRL_E_INVALID, the block untouched): handle not NULL; max_rows >= 1; block
 * not NULL and 8-byte aligned; row in [0, max_rows): a row is never wrapped; a handle that has been reset; no
 * Environment.update in progress (antsrl_update_phase).  No entry allocates or synchronises the host. */
int antsrl_stats_sizes(const AntsHandle *h, int32_t max_rows, size_t *row_bytes, size_t *scratch_bytes, size_t *bytes);
int antsrl_stats_row(AntsHandle *h, void *block, int32_t max_rows, int32_t row, void *stream);

/* The episode renderer: RGB frames of a recorded episode, computed on the device from the episode recorder's block and
 * from nothing else (the live state is not read, so no deferred update is enqueued and a running episode is not
 * disturbed; the block is read-only here).  It stands in for the reference's replay viewer (gui/visualize.py), of which
 * it reproduces ONE part bit for bit — the colour layer, the chain of mix_alpha calls (visualize.py:23-26, :220-244) —
 * and replaces the rest (pygame sprites and textures) with a composition of its own, in integers.  One call renders
 * `count` frames, frames first .. first + count - 1 of the block, for all S = n_sel recorded environments.
 *
 * view_mask: bit i is the viewer's view[i]: 0 background (dirt, anthill, walls), 1 ants, 2 explored map, 3 pheromones,
 * 4 food, 5 rocks.  ANTSRL_RENDER_VIEW_ALL sets them all; any other bit is refused.
 *
 * THE COLOUR LAYER, per cell, in float64 with every product, sum and quotient rounded on its own (no fused
 * multiply-add) and one IEEE division per channel.  It starts from rgb = (255, 255, 255), A = 0.0 and applies, in the
 * order a snapshot lists its objects (food, the pheromones 0 .. C - 1, the explored map):
 *     food         colour (64, 255, 64)       a = food / (max + 0.0001) * 0.3        view bit 4
 *                  (max: the maximum of THIS frame's food plane of this environment)
 *     pheromone k  colour phero_colors[k]     a = (phero / (phero_max_val + 0.0001)) * 0.6      view bit 3
 *     explored     colour (255, 255, 0)       a = explored / 1.0 * 0.3               view bit 2, only where the block has
 *                                                                                    the explored section
 * each as   m = A + a * (1 - A);   per channel  v = (rgb * A + (colour * a) * (1 - A)) / (m + 0.001),  rgb = (uint8) v
 * (truncated);   A = m.   After the chain alpha8 = (uint8)(A * 255).  A layer whose view bit is clear is skipped
 * entirely.  These are the reference's bytes (tests/golden/contract/render_layer_ref.npz holds its own mix_alpha's) but
 * for two cases: an explored map that is all false is 0 / 0 in the reference (it cannot occur after a recorded step);
 * here its alpha is 0 in every cell, as in any unexplored cell.  A pheromone without max_val makes the reference's
 * viewer raise; here the caller passes phero_max_val > 0 (255, where the recorder's cast saturates, is the natural one).
 *
 * THE COMPOSITION, in integers.  Image row py is y and column px is x (what pygame's surfarray shows); the cell of a
 * pixel is (px / zoom, py / zoom) — nearest-neighbour upscaling.  blend(src, a, dst) = (src * a + dst * (255 - a) +
 * 127) / 255 per channel.  Per cell, in this order: the background, dirt (134, 96, 67) under view bit 0, else black;
 * the anthill (0, 0, 255) blended at alpha 128 where (ax - x)^2 + (ay - y)^2 <= r^2, under view bit 0; the colour
 * layer blended at alpha8; a wall cell, opaque rock (96, 96, 96), under view bit 0.  Then per pixel: the rocks under
 * view bit 5, flat (150, 150, 150) where dx * dx + dy * dy <= rad * rad with dx = (px + 0.5) / zoom - cx and dy
 * likewise (float64, every operation rounded); the ants under view bit 1: ant i has its centre at ((int)(x * zoom),
 * (int)(y * zoom)) and covers the pixels with integer dx^2 + dy^2 <= ant_radius^2, in the colour ((uint8)(255 * rs /
 * 255.0), the same, (uint8)(128 * rs / 255.0)) for rs = reward_state[i] (REWARD_ANTS_COLOR * reward_state / 255), but
 * where holding[i] > 0 the pixels with dx^2 + dy^2 <= (ant_radius / 2)^2 (integer division) are (64, 255, 64).  Where
 * ants overlap the HIGHEST index wins (the reference blits in index order); ants are clipped at the image's edge.
 * There is no heading mark, no sprite, no texture and no text.
 *
 * out: uint8 [count][S][H * zoom][W * zoom][3]; with layer_only != 0 instead uint8 [count][S][W][H][4], the colour
 * layer's R, G, B and alpha8 per cell.  scratch: count * scratch_bytes_per_frame bytes (the food maxima).
 *   _sizes:   frame_env_bytes = one environment's picture of one frame (3 * W * zoom * H * zoom, or 4 * W * H with
 *             layer_only); scratch_bytes_per_frame = 4 * n_sel.  Either pointer may be NULL.  No HIP call.
 *   _frames:  two launches (the food maxima, then the frames) on `stream`.  block, n_sel, max_frames and with_heatmap are
 *             what the block was recorded with.
 * Rules, all checked before any HIP call (ANTSRL_E_INVALID, out and scratch untouched): handle, opts, block, out and
 * scratch not NULL; block, out and scratch 16-byte aligned; 1 <= n_sel <= ANTSRL_RECORDER_MAX_ENVS; max_frames >= 1;
 * 1 <= zoom <= ANTSRL_RENDER_MAX_ZOOM; 0 <= ant_radius <= ANTSRL_RENDER_MAX_ANT_RADIUS; phero_max_val > 0 (and not
 * NaN); view_mask within ANTSRL_RENDER_VIEW_ALL; first >= 0, count >= 1, first + count <= max_frames; and the launch
 * limits: count <= 65535 and groups * n_sel * count < 2^24, where groups = ceil(W / 32) * ceil(H / ty) with ty = 32
 * for zoom 1 and 2, 16 for zoom 3, 8 for zoom 4 and 5 and 4 above (a workgroup's tile of cells), or ceil(W * H /
 * 256) with layer_only — a caller with more frames splits them over several calls; and a handle that has been reset
 * (the block was recorded from it).  The entries do not allocate and do not synchronise the host. */
#define ANTSRL_RENDER_MAX_ZOOM 8
#define ANTSRL_RENDER_MAX_ANT_RADIUS 1024
#define ANTSRL_RENDER_VIEW_ALL 63
typedef struct {
    int32_t zoom, view_mask, ant_radius, layer_only;
    double phero_max_val;
    uint8_t phero_colors[4][3];
} AntsRenderOpts;
int antsrl_render_sizes(const AntsHandle *h, int32_t n_sel, const AntsRenderOpts *o,
                        size_t *frame_env_bytes, size_t *scratch_bytes_per_frame);
int antsrl_render_frames(AntsHandle *h, const void *block, int32_t n_sel, int32_t max_frames, int32_t with_heatmap,
                         int32_t first, int32_t count, const AntsRenderOpts *o, void *out, void *scratch, void *stream);

/* Copies one piece of state into a caller device buffer in the canonical
 * reference-shaped layout (ANTSRL_S_*).  Replaces attribute reads such as
 * api.ants.ants, pheromone.phero, food.qte, anthill.food. */
int antsrl_read_state(AntsHandle *h, int which, void *dst, void *stream);

/* RLApi.perceptive_field (environment/RL_api.py:144-153; main.py:51 sets save_perceptive_field for the viewer): dst
 * uint8 [E][W][H] = 1 where the perception of some ant of the environment reaches — masked cells not counted — computed from
 * the ants' positions as they stand: call it right behind antsrl_step / antsrl_observe (the reference computes it inside
 * RLApi.observation).  A deferred update (antsrl_update with the library's jitter) has not moved anything yet and is NOT
 * flushed by this call. */
int antsrl_perceptive_field(AntsHandle *h, uint8_t *dst, void *stream);

/* A CALLER'S Reward.  The reference's extension point is the Reward base class (environment/rewards/reward.py): RLApi
 * hands Reward.observation the integer cells every ant perceives (RL_api.py:164), takes the reward from Reward.step
 * (RL_api.py:202) and flashes the ants it rewards, Ants.give_reward(reward - reward_threshold) (RL_api.py:203,
 * ants.py:119-121).  A handle created with reward_kind = ANTSRL_REWARD_NONE and reward_threshold = +infinity writes a
 * reward of 0 and never flashes on its own (0 - inf > 0 is false; a built-in kind with an infinite threshold still
 * writes its reward and never flashes); these two entries then are the caller's half of RLApi.step.  They belong
 * BETWEEN the step and the update:
 *     antsrl_step;  antsrl_obs_coords;  <the caller's reward>;  antsrl_give_reward;  antsrl_update
 * — the reference gives the reward before Environment.update decays reward_state (ants.py:130).  Towards the handle
 * both behave alike: a handle that was never reset is refused, so is one between two phases of antsrl_update_phase
 * (they are no mere reads of a half-updated world), and a DEFERRED update is enqueued first (the coordinates are then
 * those of the ants where that update left them, and the 255 lands on the decayed reward_state).  Neither allocates
 * nor synchronises the host.
 *
 * antsrl_obs_coords: dst int32 [E][N][P][P][2] (8-byte aligned) = abs_coords of RL_api.py:100-119 for the ants as they
 * stand: the centre shifted by fwd_delta along the heading, the grid's offsets times delta rotated by theta + pi / 2,
 * rounded half to even, wrapped onto the torus; pair (x, y) of row i, column j belongs to the offset perception_coords
 * [i][j] = ((j - r) * delta, (i - r) * delta), the order of the observation's cells.  MASKED offsets are included, as in
 * the reference: the caller applies the mask.
 *
 * antsrl_give_reward: reward float64 [E][N].  reward_state[a] = 255 where reward[a] - threshold > 0, evaluated in
 * float64; reward_out (float32 [E][N], may be NULL) takes (float)reward[a] — pass the step's reward buffer and whoever
 * reads it afterwards sees the caller's reward. */
int antsrl_obs_coords(AntsHandle *h, int32_t *dst, void *stream);
int antsrl_give_reward(AntsHandle *h, const double *reward, double threshold, float *reward_out, void *stream);

/* Size in bytes of what antsrl_read_state(which) writes. */
int antsrl_state_bytes(const AntsHandle *h, int which, size_t *bytes);

/* The population of linear agents: P CollectAgents (the net of "The linear agent's training step": layer1 frozen, layer2
 * and layer3 trained, 198 floats) trained in lockstep on ONE handle, with one launch per stage of the agent's loop
 * whatever P is.  Member p owns environments [p Em, (p + 1) Em) of the handle's n_envs = P Em, that is ants
 * [p Mm, (p + 1) Mm) of the batch's flat order, Mm = Em n_ants.
 *
 * THE DEFINING PROPERTY.  Member p is, bit for bit, the single agent's entries (antsrl_policy_mlp,
 * antsrl_agent_select_actions, antsrl_replay_record_pre_plain / _post_plain, antsrl_lintrain_step) run on a handle of
 * those Em environments created with env_id_base = env_id_base + p Em, with the member's own seed, epsilon, discount
 * and learning rate: actions, explored flags, ring rows, heads, Adam's moments, gradients and loss.  Each kernel here is
 * the single agent's stage with the member taken from the grid, and runs the same body text as the single agent's kernel
 * (one .inc file per body, included in both: antsrl_population.hip); every draw of the draw specification is keyed on the GLOBAL environment id.
 *
 * Layout: member-major device tensors, a member's block laid out exactly as the single agent's:
 *   w1 float [P][32][F + 2], b1 float [P][32]       the frozen layer1 (a member may have its own)
 *   heads float [P][198], target_l3 float [P][99]   as antsrl_lintrain_*'s heads and target_l3
 *   adam float [P][2][198]                          a member's m, then its v
 *   grads float [P][198], loss float [P]
 *   the ring: the seven arrays of antsrl_replay_record_* with a leading [P] (states float [P][max_len][F], ...); head
 *   and fill are ONE pair of host numbers, because every member records the same K rows at every step
 *   obs [P][Mm][F] (= the handle's [n_envs][n_ants][F]), agent_state float [P][Mm][2], rotation / pheromone int8 [P][Mm],
 *   reward float [P][Mm], done / explored uint8 [P][Em]: the handle's own buffers
 *
 * The table: the per-member hyper-parameters (seed, epsilon, discount, learning_rate) are HOST values in
 * AntsPopSpec.members; an entry hands them to its kernel by value in the kernel's arguments, so changing an epsilon
 * between steps costs no device allocation and no copy.  At most ANTSRL_POP_MAX = 64 members (about 1.5 KB of
 * arguments).  Common to all members: Adam's betas, eps and step count, B, K, the ring's max_len.
 *
 * THE ALIGNMENT RULE (antsrl_pop_policy only).  The acting kernel streams each 32-ant tile of a member's rows as 16-byte
 * pieces from the tile's first byte; tile t of member p starts (p Mm + 32 t) F elements behind obs.  Tiles within a member
 * are 64 F (bfloat16) or 128 F (float32) bytes apart, always multiples of 16, so what is needed is that every MEMBER's
 * slice starts 16-byte aligned: obs 16-byte aligned and
 *     Em * n_ants * n_features * sizeof(element)  a multiple of 16.
 * (The single agent's rows start at obs, so it never meets the rule.)  antsrl_pop_select reads no observation, and the
 * record entries copy rows at whatever alignment they have, as antsrl_replay_record_* do.
 * Only the flat form of the acting kernel is offered: an n_features whose W1 and two 32-row images do not fit 160 KiB
 * of LDS (antsrl_policy_mlp's fallback case) is ANTSRL_E_UNSUPPORTED.  Observation rows are dense: obs_pitch is 0 or
 * n_features.
 *
 * Refusals, each in words and before anything is launched (ANTSRL_E_INVALID unless stated):
 *   a NULL spec; n_members outside [1, ANTSRL_POP_MAX]; n_envs, n_ants, env_id_base outside the rules of
 *   antsrl_agent_select; n_envs not a multiple of n_members; n_features < 1, or n_features + 2 > 1024 (UNSUPPORTED); an
 *   obs_format that is neither ANTSRL_OBS_F32 nor ANTSRL_OBS_BF16; an obs_pitch other than 0 or n_features
 *   (UNSUPPORTED); a member's epsilon outside [0, 1] or NaN discount;
 *   antsrl_pop_policy: the flat form does not take n_features (UNSUPPORTED); the alignment rule (UNSUPPORTED); obs not
 *     16-byte aligned; any NULL or misaligned pointer (pheromone included: the net has both heads);
 *   antsrl_pop_select: NULL rotation or pheromone (explored may be NULL);
 *   antsrl_pop_record_*: K outside [1, Em n_ants]; max_len outside [1, 2^40]; head outside [0, max_len); any NULL or
 *     misaligned pointer (pheromone may be NULL, as for antsrl_replay_record_pre);
 *   antsrl_pop_lintrain_step: B < 1; B > 512 (UNSUPPORTED: a member's step is one workgroup, antsrl_lintrain_step's
 *     one-launch form); n_rows outside [1, 2^40]; any NULL or misaligned pointer (idx is required, grads and
 *     running_loss may be NULL); Adam's arguments as antsrl_lintrain_step's, for every member's learning_rate.
 * No entry allocates or synchronises the host; there are no atomics: equal inputs give equal bits.  One launch each.
 *
 *   antsrl_pop_policy     the acting net of every member on its own rows: rotation = argmax(layer2(h)) - 1 with the
 *                         member's live layer2 (heads [p][0 .. 99)), pheromone = argmax(layer3(h)) with its TARGET layer3
 *                         (target_l3 [p]): the net CollectAgent.get_action acts with.  Grid (blocks, P): a workgroup
 *                         stages one member's W1 and loops over that member's tiles only.
 *   antsrl_pop_select     antsrl_agent_select_actions per member, n_rot = n_ph = 3: environment e of member p explores
 *                         iff u01(draw(seed_p, ANTSRL_DRAW_EXPLORE, env_id_base + p Em + e, step, 0)) < epsilon_p.
 *   antsrl_pop_record_*   antsrl_replay_record_*_plain per member (agent_dim 2, n_rot 3): K of the member's Mm
 *                         transitions, sampled with draw(seed_p, ANTSRL_DRAW_SAMPLE, env_id_base + p Em, step, j), into
 *                         rows (head + j) mod max_len of the member's slab.  Grid (ceil(K / 4), P).
 *   antsrl_pop_lintrain_step   antsrl_lintrain_step per member, one workgroup each, grid (1, P): idx int64 [P][B], row p
 *                         indexing member p's slab (clamped to [0, n_rows); n_rows is also the slab's stride in rows:
 *                         pass max_len); discount_p; Adam with lr_p at the common step count.  running_loss (double [P],
 *                         or NULL): the same launch then also keeps main.py:106-109's recurrence per member in float64,
 *                         running_loss[p] = loss[p] when first_loss != 0 (the host knows its first training step), else
 *                         0.99 * running_loss[p] + 0.01 * loss[p], each product rounded before the add
 *                         (antsrl_monitor_step's arithmetic).
 * The target sync is one device copy of [P][99] (heads [.][99 .. 198) into target_l3), the caller's. */
#define ANTSRL_POP_MAX 64

typedef struct AntsPopMember {
    uint64_t seed;
    double epsilon;
    double learning_rate;
    float discount;
    int32_t reserved; /* 0 */
} AntsPopMember;

typedef struct AntsPopSpec {
    int32_t n_members;                  /* P */
    int32_t n_envs, n_ants, env_id_base; /* the whole handle's: Em = n_envs / n_members */
    int32_t n_features;
    int32_t obs_format;                 /* ANTSRL_OBS_F32 / ANTSRL_OBS_BF16 */
    int32_t obs_pitch;                  /* 0 or n_features */
    int32_t reserved;                   /* 0 */
    AntsPopMember members[ANTSRL_POP_MAX];
} AntsPopSpec;

int antsrl_pop_policy(const AntsPopSpec *s, const void *obs, const float *agent_state, const float *w1, const float *b1,
                      const float *heads, const float *target_l3, int8_t *rotation, int8_t *pheromone, void *stream);
int antsrl_pop_select(const AntsPopSpec *s, uint64_t step, int8_t *rotation, int8_t *pheromone, uint8_t *explored,
                      void *stream);
int antsrl_pop_record_pre(const AntsPopSpec *s, uint64_t step, int64_t K, int64_t head, int64_t max_len, const void *obs,
                          const float *agent_state, const int8_t *rotation, const int8_t *pheromone, float *states,
                          float *agent_states, int64_t *actions, void *stream);
int antsrl_pop_record_post(const AntsPopSpec *s, uint64_t step, int64_t K, int64_t head, int64_t max_len, const void *obs,
                           const float *agent_state, const float *reward, const uint8_t *done, float *rewards,
                           float *new_states, float *new_agent_states, uint8_t *dones, void *stream);
int antsrl_pop_lintrain_step(const AntsPopSpec *s, const float *w1, const float *b1, float *heads, const float *target_l3,
                             float *adam, const float *states, const float *agent_states, const int64_t *actions,
                             const float *rewards, const float *new_states, const float *new_agent_states,
                             const uint8_t *dones, int64_t n_rows, const int64_t *idx, int64_t B, int64_t step, double beta1,
                             double beta2, double eps, float *grads, float *loss, double *running_loss, int first_loss,
                             void *stream);

/* The population of explore agents: P ExploreAgents (the net of "The explore agent's training step": layer1 and layer2
 * both trained, the target net a full copy) in lockstep on one handle — the first stage of the curriculum whose second
 * stage is the population above.  The spec, the members' shares of the handle, the table and the alignment rule are that
 * population's; so are select and record: antsrl_pop_select draws a pheromone that nothing reads, and
 * antsrl_pop_record_pre with pheromone = NULL stores (rotation + 1, 1).
 *
 * THE DEFINING PROPERTY is the same: member p is, bit for bit, antsrl_policy_mlp without a pheromone head (w3 = NULL) on
 * its TARGET block, antsrl_agent_select_actions, antsrl_replay_record_*_plain and antsrl_exptrain_step run on a handle of
 * its Em environments, with its own seed, epsilon, discount and learning rate.
 *
 * Layout: model, target, adam_m, adam_v, grads float [P][T], T = 32 (F + 2) + 131 (antsrl_exptrain_sizes'
 * trained_floats), a member's block laid out as antsrl_exptrain_step's; loss float [P]; idx int64 [P][B]; the ring as
 * above.  T is odd for an even F, so a member's block is 4-byte aligned and no more: the kernels read and write the
 * blocks one float at a time.  The workspace is member-major: member p's part starts p * workspace_stride bytes behind
 * `workspace` and is laid out as antsrl_exptrain_step's (partials, then dh [B][32]); workspace_stride is that entry's
 * workspace_bytes rounded up to 256.
 *
 * Refusals (ANTSRL_E_INVALID unless stated), before anything is launched: the spec's, as above;
 *   antsrl_pop_explore_policy: the flat form does not take n_features (UNSUPPORTED); the alignment rule (UNSUPPORTED);
 *     obs not 16-byte aligned; any NULL or misaligned pointer;
 *   antsrl_pop_exptrain_sizes: n_features as above; B < 1; B > 512 (UNSUPPORTED); n_members outside [1, ANTSRL_POP_MAX];
 *   antsrl_pop_exptrain_step: B < 1; B > 512 (UNSUPPORTED: at most four workgroups of the forward stage per member and
 *     256 in all); n_rows outside [1, 2^40]; any NULL or misaligned pointer (idx is required and 8-byte aligned; the
 *     workspace 256-byte aligned; grads and running_loss may be NULL, running_loss 8-byte aligned); Adam's arguments for
 *     every member's learning_rate.
 * No entry allocates or synchronises the host; no atomics: equal inputs give equal bits.
 *
 *   antsrl_pop_explore_policy  rotation = argmax(layer2(h)) - 1 of every member's TARGET block (target_blocks [P][T]) on
 *                         its own rows.  One launch, grid (blocks, P), antsrl_pop_policy's launch rule.
 *   antsrl_pop_exptrain_sizes  trained_floats = T, workspace_stride, workspace_bytes = n_members * workspace_stride and
 *                         launches = 2 (any of the four may be NULL).
 *   antsrl_pop_exptrain_step   antsrl_exptrain_step per member in TWO launches: the forward stage on grid
 *                         (ceil(B / 128), P), the layer1 stage on grid (ceil((F + 3) / 8) + 1, P).  idx, n_rows, step,
 *                         running_loss and first_loss as antsrl_pop_lintrain_step's; the second launch keeps the
 *                         running loss.
 * The target sync is one device copy of [P][T] (model into target), the caller's; the hand-over to the population of
 * linear agents is a device copy per member of the model block's layer1 and layer2 into w1, b1 and heads [p][0 .. 99). */
int antsrl_pop_explore_policy(const AntsPopSpec *s, const void *obs, const float *agent_state, const float *target_blocks,
                              int8_t *rotation, void *stream);
int antsrl_pop_exptrain_sizes(int32_t n_features, int64_t B, int32_t n_members, size_t *trained_floats,
                              size_t *workspace_stride, size_t *workspace_bytes, int32_t *launches);
int antsrl_pop_exptrain_step(const AntsPopSpec *s, float *model, const float *target, float *adam_m, float *adam_v,
                             const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                             const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                             const int64_t *idx, int64_t B, int64_t step, double beta1, double beta2, double eps,
                             float *grads, float *loss, double *running_loss, int first_loss, void *workspace,
                             void *stream);

/* The population of joint agents: P CollectAgents with the freeze of layer1 lifted (the net of "The joint training
 * step": all six tensors trained, layer1 and layer2 live in model and target net, layer3 with a target copy) in lockstep
 * on one handle — the third stage of the curriculum whose first two stages are the populations above.  The spec, the
 * members' shares of the handle, the table and the alignment rule are the population of linear agents'; so are select
 * and record, unchanged: the net has both heads and the ring stores both actions.
 *
 * THE DEFINING PROPERTY is the same: member p is, bit for bit, antsrl_policy_mlp on layer1 and layer2 of its LIVE model
 * block and its TARGET layer3, antsrl_agent_select_actions, antsrl_replay_record_*_plain and antsrl_jointtrain_step run
 * on a handle of its Em environments, with its own seed, epsilon, discount and learning rate.
 *
 * Layout: model, adam_m, adam_v, grads float [P][T], T = 32 (F + 2) + 230 (antsrl_jointtrain_sizes' trained_floats), a
 * member's block laid out as antsrl_jointtrain_step's (w1 | b1 | w2 | b2 | w3 | b3); target_l3 float [P][99]; loss float
 * [P]; idx int64 [P][B]; the ring as above.  A member's block and its target layer3 (99 floats) are 4-byte aligned and
 * no more: the kernels read and write the blocks one float at a time.  The workspace is member-major: member p's part
 * starts p * workspace_stride bytes behind `workspace` and is laid out as antsrl_jointtrain_step's (partials, then dh
 * [B][32]); workspace_stride is that entry's workspace_bytes rounded up to 256.
 *
 * Refusals (ANTSRL_E_INVALID unless stated), before anything is launched: the spec's, as above;
 *   antsrl_pop_joint_policy: the flat form does not take n_features (UNSUPPORTED); the alignment rule (UNSUPPORTED);
 *     obs not 16-byte aligned; any NULL or misaligned pointer (pheromone included: the net has both heads);
 *   antsrl_pop_jointtrain_sizes: n_features as above; B < 1; B > 512 (UNSUPPORTED); n_members outside [1, ANTSRL_POP_MAX];
 *   antsrl_pop_jointtrain_step: B < 1; B > 512 (UNSUPPORTED: at most four workgroups of the forward stage per member and
 *     256 in all); n_rows outside [1, 2^40]; any NULL or misaligned pointer (idx is required and 8-byte aligned; the
 *     workspace 256-byte aligned; grads and running_loss may be NULL, running_loss 8-byte aligned); Adam's arguments for
 *     every member's learning_rate.
 * No entry allocates or synchronises the host; no atomics: equal inputs give equal bits.
 *
 *   antsrl_pop_joint_policy    rotation = argmax(layer2(h)) - 1 and pheromone = argmax(layer3(h)) of every member on its
 *                         own rows: w1, b1, w2, b2 of its LIVE block (model_blocks [P][T]), w3, b3 of its target_l3 [p].
 *                         One launch, grid (blocks, P), antsrl_pop_policy's launch rule.
 *   antsrl_pop_jointtrain_sizes  trained_floats = T, workspace_stride, workspace_bytes = n_members * workspace_stride and
 *                         launches = 2 (any of the four may be NULL).
 *   antsrl_pop_jointtrain_step   antsrl_jointtrain_step per member in TWO launches: the forward stage on grid
 *                         (ceil(B / 128), P), the layer1 stage on grid (ceil((F + 3) / 8) + 1, P).  idx, n_rows, step,
 *                         running_loss and first_loss as antsrl_pop_lintrain_step's; the second launch keeps the
 *                         running loss.
 * The target sync is one device copy of [P][99] (model [.][T - 99 .. T) into target_l3), the caller's; the hand-over
 * from the population of linear agents is a device copy per tensor of w1, b1 and heads into the model block (w1 at 0,
 * b1 at 32 (F + 2), heads behind it) and of heads [.][99 .. 198) into target_l3. */
int antsrl_pop_joint_policy(const AntsPopSpec *s, const void *obs, const float *agent_state, const float *model_blocks,
                            const float *target_l3, int8_t *rotation, int8_t *pheromone, void *stream);
int antsrl_pop_jointtrain_sizes(int32_t n_features, int64_t B, int32_t n_members, size_t *trained_floats,
                                size_t *workspace_stride, size_t *workspace_bytes, int32_t *launches);
int antsrl_pop_jointtrain_step(const AntsPopSpec *s, float *model, const float *target_l3, float *adam_m, float *adam_v,
                               const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                               const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                               const int64_t *idx, int64_t B, int64_t step, double beta1, double beta2, double eps,
                               float *grads, float *loss, double *running_loss, int first_loss, void *workspace,
                               void *stream);

/* The population of memory nets: the DQN training step of P memory agent nets (the net of antsrl_memtrain_*, the agent
 * main.py drives) in the launches of ONE step: 16 + 1 = 17 whatever P is, each the single step's kernel on a grid
 * (x, P) with the member in the grid's y dimension; and behind it the rest of the memory agents' loop for a population
 * (antsrl_pop_policy_memory, antsrl_pop_memory_select, antsrl_pop_memory_record_pre / _post, below).  The spec is the
 * population of linear agents' (the training entry reads its members' discount and learning_rate and its n_features,
 * which must be the shape's).
 *
 * THE DEFINING PROPERTY: member p is, bit for bit, antsrl_memtrain_grad followed by antsrl_memtrain_apply on its own
 * state blocks, ring slab and idx row, with its own discount and learning rate; its result does not depend on P or on
 * the other members' data.
 *
 * Layout: net_states and target_states are [P][state_stride] bytes, a member's block laid out as antsrl_memtrain_*'s
 * state (state_stride is antsrl_memtrain_sizes' state_bytes); antsrl_memtrain_init / _unpack / _copy work on a member
 * at net_states + p * state_stride.  The workspace is [P][work_stride] bytes, a member's part laid out as
 * antsrl_memtrain_grad's (work_stride is antsrl_memtrain_sizes' workspace_bytes).  Both strides are multiples of 256, so
 * that every member's blocks start as aligned as a single net's.  The ring's seven arrays have a leading [P] of n_rows
 * rows each (agent_states and new_agent_states [P][n_rows][agent_dim + mem_size]); idx int64 [P][B], required, every
 * value in [0, n_rows); grads float [P][trained_floats]; loss float [P]; running_loss double [P] or NULL.
 *
 * Refusals (ANTSRL_E_INVALID unless stated), before anything is launched: the spec's, as above; the shape's, as
 * antsrl_memtrain_sizes' (a NULL shape; D = n_features + agent_dim + mem_size > 1024 is UNSUPPORTED);
 *   antsrl_pop_memtrain_sizes: B outside [1, 2^24]; n_members outside [1, ANTSRL_POP_MAX];
 *   antsrl_pop_memtrain_step: the spec's n_features is not the shape's; B < 1; net_states, target_states or workspace
 *     NULL or not 256-byte aligned; idx NULL or not 8-byte aligned; n_rows outside [1, 2^40]; any ring array, grads or
 *     loss NULL or misaligned (floats 4 bytes, actions 8); running_loss not 8-byte aligned; step < 1 and Adam's other
 *     arguments for every member's learning_rate.
 * No entry allocates or synchronises the host; no atomics: equal inputs give equal bits.
 *
 *   antsrl_pop_memtrain_sizes  state_stride, trained_floats, work_stride, workspace_bytes = n_members * work_stride and
 *                         launches = 17 (any of the five may be NULL).  Host only.
 *   antsrl_pop_memtrain_step   the step of every member: gradient and loss (16 launches), then Adam with the member's
 *                         step size and the repack (1 launch).  step, beta1, beta2, eps, running_loss and first_loss as
 *                         antsrl_pop_lintrain_step's; the finalize launch keeps the running loss.
 * The target sync is antsrl_memtrain_copy per member, the caller's. */
int antsrl_pop_memtrain_sizes(const AntsMemNetShape *shape, int64_t B, int32_t n_members, size_t *state_stride,
                              size_t *trained_floats, size_t *work_stride, size_t *workspace_bytes, int32_t *launches);
int antsrl_pop_memtrain_step(const AntsPopSpec *s, const AntsMemNetShape *shape, void *net_states, const void *target_states,
                             const float *states, const float *agent_states, const int64_t *actions, const float *rewards,
                             const float *new_states, const float *new_agent_states, const uint8_t *dones, int64_t n_rows,
                             const int64_t *idx, int64_t B, int64_t step, double beta1, double beta2, double eps,
                             float *grads, float *loss, double *running_loss, int first_loss, void *workspace,
                             void *stream);

/* The population of memory nets, the loop around the step: acting with one pack per member, the epsilon-greedy select
 * that gives exploring ants their old memory back, and the ring's two record halves with the carried memory.  One
 * launch per entry whatever P is.  Em = n_envs / n_members, Mm = Em * n_ants; member p owns environments
 * [p Em, (p + 1) Em) and ants [p Mm, (p + 1) Mm) of every array, as in the populations above.
 *
 * THE DEFINING PROPERTY: member p computes, bit for bit, what antsrl_policy_memory, antsrl_agent_select and
 * antsrl_replay_record_pre / _post compute on its own slice with its own pack, seed and epsilon and env_id_base + p Em;
 * no output of a member depends on P or on another member's data.
 *
 * Layout: packed is [P][pack_stride] bytes, a member's block what antsrl_memnet_pack_ex(ANTSRL_MEMNET_BF16) writes at
 * packed + p * pack_stride (the caller packs a member when its acting weights change: P calls, not on the hot path);
 * pack_stride is antsrl_memnet_packed_bytes' value, a multiple of 256 (checked, not assumed).  obs [P][Mm][n_features]
 * dense; agent_state [P][Mm][agent_dim]; mem_in, mem_out, mem_old, mem_next, memory [P][Mm][mem_size]; rotation,
 * pheromone [P][Mm]; q_out [P][Mm][n_rot + n_ph] or NULL; explored [n_envs] or NULL; the ring's arrays with a leading
 * [P] of max_len rows, agent_states and new_agent_states rows agent_dim + mem_size floats wide.
 *
 * Precision: bf16 operands only.  An unknown precision is ANTSRL_E_INVALID, before any other check;
 * ANTSRL_MEMNET_FP32 is ANTSRL_E_UNSUPPORTED (a population acts with the bf16 forward).
 *
 * Refusals (ANTSRL_E_INVALID unless stated), each in words and before any HIP call: a NULL spec or shape; the spec's
 * rules, as above; the shape's, as antsrl_memnet_packed_bytes'; the spec's n_features is not the shape's; n_members
 * outside [1, ANTSRL_POP_MAX]; Mm above 2^31 - 1 - 128, beyond which the tile count of a member's grid row does not fit
 * an int (UNSUPPORTED); a pack stride that is not a multiple of 256 (UNSUPPORTED); packed NULL or not 256-byte
 * aligned; obs, agent_state, mem_in, mem_out, rotation NULL, a float array not 4-byte aligned (bfloat16 obs: 2),
 * actions not 8-byte aligned; mem_old and mem_next overlapping without being equal; for the record pair the ring rules
 * of antsrl_pop_record_pre (K in [1, Mm], max_len in [1, 2^40], head in [0, max_len)) and memory NULL.
 *
 *   antsrl_pop_memnet_sizes    pack_stride and packed_bytes = n_members * pack_stride (either may be NULL).  Host only.
 *   antsrl_pop_policy_memory   every member's net on its rows: rotation (argmax - n_rot / 2), pheromone (may be NULL),
 *                         the new memory into mem_out (mem_in == mem_out is allowed: in place, as the single entry)
 *                         and, when q_out is not NULL, both heads' outputs.  Grid (ceil(Mm / 128), P) at D <= 320.
 *   antsrl_pop_memory_select   antsrl_agent_select per member with the member's seed and epsilon: the ants of an
 *                         exploring environment take uniform actions and, unless mem_old == mem_next, their rows of
 *                         mem_next become mem_old's.  n_rot, n_ph and mem_size are the shape's.  explored may be NULL.
 *   antsrl_pop_memory_record_pre / _post   antsrl_pop_record_pre / _post with agent_dim, mem_size and n_rot / 2 from the
 *                         shape and `memory` behind agent_state in every ring row.  (The pair without a shape keeps
 *                         writing agent_dim = 2 wide rows and takes no memory.) */
int antsrl_pop_memnet_sizes(const AntsMemNetShape *shape, int precision, int32_t n_members, size_t *pack_stride,
                            size_t *packed_bytes);
int antsrl_pop_policy_memory(const AntsPopSpec *s, const AntsMemNetShape *shape, int precision, const void *packed,
                             const void *obs, const float *agent_state, const float *mem_in, float *mem_out,
                             int8_t *rotation, int8_t *pheromone, float *q_out, void *stream);
int antsrl_pop_memory_select(const AntsPopSpec *s, const AntsMemNetShape *shape, uint64_t step, int8_t *rotation,
                             int8_t *pheromone, const float *mem_old, float *mem_next, uint8_t *explored, void *stream);
int antsrl_pop_memory_record_pre(const AntsPopSpec *s, const AntsMemNetShape *shape, uint64_t step, int64_t K, int64_t head,
                                 int64_t max_len, const void *obs, const float *agent_state, const float *memory,
                                 const int8_t *rotation, const int8_t *pheromone, float *states, float *agent_states,
                                 int64_t *actions, void *stream);
int antsrl_pop_memory_record_post(const AntsPopSpec *s, const AntsMemNetShape *shape, uint64_t step, int64_t K, int64_t head,
                                  int64_t max_len, const void *obs, const float *agent_state, const float *memory,
                                  const float *reward, const uint8_t *done, float *rewards, float *new_states,
                                  float *new_agent_states, uint8_t *dones, void *stream);

/* The population of rework agents: P CollectAgentReworks (the net of "The rework agent's net" and "The rework agent's
 * training step") in lockstep on one handle.  The collapse of every member's target net is ONE launch, the acting net
 * with or without the epsilon-greedy select ONE launch and the training step the single step's FOUR launches, each on
 * a grid (x, P) with the member in the grid's y dimension, whatever P is.  The spec is the population of linear
 * agents'; Em = n_envs / n_members, Mm = Em * n_ants; member p owns environments [p Em, (p + 1) Em) and ants
 * [p Mm, (p + 1) Mm).  Members share one AntsReworkShape (hidden widths, n_rot and n_ph, 1 .. 8 each).  The select
 * without the fusion and the ring's two record halves are the population of linear agents' (antsrl_pop_select,
 * antsrl_pop_record_pre / _post: three-wide heads, rotation + 1 stored).
 *
 * THE DEFINING PROPERTY: member p computes, bit for bit, what antsrl_rework_collapse, antsrl_policy_rework,
 * antsrl_policy_rework_select (seed, epsilon of the member, env_id_base + p Em) and antsrl_reworktrain_step (discount and
 * learning rate of the member) compute on its own block, collapsed buffer, rows, ring slab and idx row; no output of a
 * member depends on P or on another member's data.  A member with epsilon 0 is evaluated on every row by the select
 * entry and gets antsrl_policy_rework's bits.
 *
 * Layout: NF = antsrl_reworktrain_sizes' params_floats, CF = (n_rot + n_ph) * (n_features + 2) + n_rot + n_ph.  model,
 * target_blocks, adam_m, adam_v and grads are float [P][NF], a member's block the single trainer's (the 20 tensors of
 * the state_dict in its order); collapsed and target_collapsed float [P][CF], a member's buffer what
 * antsrl_rework_collapse writes.  Blocks and buffers are 4-byte aligned and no more (neither count is a multiple of 4 in
 * general).  obs [P][Mm][n_features] dense, a member's slice a multiple of 16 bytes; agent_state [P][Mm][2]; rotation,
 * pheromone [P][Mm]; q_out [P][Mm][n_rot + n_ph] or NULL; explored [n_envs] or NULL.  The workspace is
 * [P][workspace_stride] bytes, a member's part laid out as antsrl_reworktrain_step's for the same B; the stride is a
 * multiple of 256 and at least antsrl_reworktrain_sizes' workspace_bytes.  The ring's seven arrays have a leading [P] of
 * n_rows rows each; idx int64 [P][B], required, every value in [0, n_rows); loss float [P]; running_loss double [P] or
 * NULL.
 *
 * Refusals (ANTSRL_E_INVALID unless stated), each in words and before any launch: a NULL spec or shape; the spec's
 * rules, as above; the shape's, as antsrl_rework_collapse's (a head wider than 8, a hidden width above 256 and
 * n_features + 2 > 1024 are UNSUPPORTED); the spec's n_features is not the shape's; n_members outside
 * [1, ANTSRL_POP_MAX]; a member's observation slice that is no multiple of 16 bytes (UNSUPPORTED);
 *   the acting entries: collapsed, agent_state or q_out not 4-byte aligned, obs not 16-byte aligned, any of them but
 *     q_out NULL, rotation or pheromone NULL;
 *   antsrl_pop_reworktrain_sizes / _step: B outside [1, 65536] (above: UNSUPPORTED); model, target_collapsed, adam_m or
 *     adam_v NULL or not 4-byte aligned; idx NULL or not 8-byte aligned; workspace NULL or not 256-byte aligned; n_rows
 *     outside [1, 2^40]; any ring array, grads or loss NULL or misaligned; running_loss not 8-byte aligned; step < 1 and
 *     Adam's other arguments for every member's learning_rate.
 * No entry allocates or synchronises the host; no atomics: equal inputs give equal bits.
 *
 *   antsrl_pop_rework_collapse       collapsed[p] = antsrl_rework_collapse of block p of target_blocks.  Grid (NQ, P).
 *   antsrl_pop_policy_rework         every member's collapsed net on its rows: rotation (argmax - n_rot / 2), pheromone
 *                         and, when q_out is not NULL, both heads' outputs.
 *   antsrl_pop_policy_rework_select  the same and antsrl_pop_select's epsilon-greedy in one launch, among n_rot and n_ph
 *                         actions, without the forward pass of the rows whose whole pass explores; q_out is written
 *                         for the rows of the other colonies only.
 *   antsrl_pop_reworktrain_sizes     trained_floats = NF, collapsed_floats = CF, workspace_stride, workspace_bytes =
 *                         n_members * workspace_stride and launches = 4 (any of the five may be NULL).  Host only.
 *   antsrl_pop_reworktrain_step      the step of every member: down chain, batch pass, up chain (which keeps the running
 *                         loss), gradient and Adam with the member's step size.  step, beta1, beta2, eps, running_loss
 *                         and first_loss as antsrl_pop_lintrain_step's.  target_collapsed is read, never written.
 * The target sync is one copy of [P][NF] and one antsrl_pop_rework_collapse, the caller's. */
int antsrl_pop_rework_collapse(const AntsReworkShape *shape, int32_t n_members, const float *target_blocks, float *collapsed,
                               void *stream);
int antsrl_pop_policy_rework(const AntsPopSpec *s, const AntsReworkShape *shape, const void *collapsed, const void *obs,
                             const float *agent_state, int8_t *rotation, int8_t *pheromone, float *q_out, void *stream);
int antsrl_pop_policy_rework_select(const AntsPopSpec *s, const AntsReworkShape *shape, const void *collapsed, const void *obs,
                                    const float *agent_state, uint64_t step, int8_t *rotation, int8_t *pheromone,
                                    uint8_t *explored, float *q_out, void *stream);
int antsrl_pop_reworktrain_sizes(const AntsReworkShape *shape, int64_t B, int32_t n_members, size_t *trained_floats,
                                 size_t *collapsed_floats, size_t *workspace_stride, size_t *workspace_bytes,
                                 int32_t *launches);
int antsrl_pop_reworktrain_step(const AntsPopSpec *s, const AntsReworkShape *shape, float *model, const float *target_collapsed,
                                float *adam_m, float *adam_v, const float *states, const float *agent_states,
                                const int64_t *actions, const float *rewards, const float *new_states,
                                const float *new_agent_states, const uint8_t *dones, int64_t n_rows, const int64_t *idx,
                                int64_t B, int64_t step, double beta1, double beta2, double eps, float *grads, float *loss,
                                double *running_loss, int first_loss, void *workspace, void *stream);

/* Population-based training: what a loop that ranks the members of any of the five populations, copies a winner over a
 * loser and perturbs the loser's hyper-parameters needs of the device (antsrl_amd/pbt.py holds the loop's host side;
 * DESIGN 7.35).  Both entries validate every argument on the host before any HIP call and enqueue ONE launch on the
 * caller's stream; neither allocates or synchronises.
 *
 * antsrl_pop_fitness: row[p] = {total, min, max} of member p's episode reward, p = 0 .. n_members - 1 (double
 * [n_members][3]).  episode_reward is the monitor block's double [n_envs][n_ants] ("The training monitor"); it is read,
 * never written.  Member p owns environments [p Em, (p + 1) Em), Em = n_envs / n_members.  `total` is over the member's
 * ants; min and max are over its environments' totals.  One workgroup of 256 per member, grid n_members.
 * THE ORDER OF THE SUMS is the monitor's (antsrl_monitor.h), every add a float64 add, round to nearest even:
 *     an environment's total:  the total[e] rule: slot t starts at +0.0 and adds episode_reward[e][n] for n = t, t + 256,
 *                              t + 512, ... ascending; the 256 slots are folded with x[i] += x[i + s] for i < s,
 *                              s = 128, 64, ..., 1; total = x[0].
 *     the member's total:      the same rule over its Em environment totals: slot t takes environments t, t + 256, ...
 *                              of the member.
 *     min / max:               order-free.
 * So a member's total is reproducible bit for bit, and it equals the grand_total rule applied to the member's
 * environments of a monitor's report taken at the same step.  Nothing here is float32.
 * ANTSRL_E_INVALID, each with its own message: a NULL or not 8-byte aligned episode_reward or row; n_members outside
 * [1, ANTSRL_POP_MAX]; n_envs < 1 or n_ants < 1; n_envs no multiple of n_members; row overlapping episode_reward.
 *
 * antsrl_pop_exploit: array a (a = 0 .. n_arrays - 1) is [n_members] rows of row_bytes[a] bytes at base[a], members
 * outermost; for every pair i, row src[i] of EVERY array is copied over row dst[i].  One launch of the table-driven copy
 * behind antsrl_fork_envs whatever n_arrays and n_pairs are: 16 bytes per lane where a pair's two rows are congruent
 * modulo 16, 4 bytes where they are congruent modulo 4 only (a member's block of 9603 floats), single bytes otherwise;
 * no byte outside a destination row is written and none outside a source row is read.  base and row_bytes are host
 * arrays; src and dst are host arrays too.  A src may repeat (one winner over several losers).  The arrays must not
 * overlap each other (not checked).
 * ANTSRL_E_INVALID, each with its own message: n_arrays outside [1, 40]; n_pairs outside [0, 640] (n_pairs == 0 returns
 * ANTSRL_OK and launches nothing); n_members outside [1, ANTSRL_POP_MAX]; NULL base or row_bytes; a row_bytes of 0; a
 * NULL base[a]; NULL src or dst; an index outside [0, n_members); a dst that repeats; a dst that is also a src (so no
 * row is read and written in one launch). */
int antsrl_pop_fitness(const double *episode_reward, int n_envs, int n_ants, int n_members, double *row, void *stream);
int antsrl_pop_exploit(int n_arrays, void *const *base, const uint64_t *row_bytes, int n_members, int n_pairs,
                       const int32_t *src, const int32_t *dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ANTSRL_H */
