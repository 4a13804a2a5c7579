#!/usr/bin/env python3
"""Generates the golden fixtures under tests/golden/*.npz by RUNNING THE REFERENCE.

Run in the build container only (the reference lives at /root/reference there and never
travels):   python tests/golden/make_golden.py

The reference is imported unmodified with the two in-process shims of SURVEY.md §8(c):
a dummy ``noise`` module (imported but unused on this path) and ``np.bool`` (alias removed
from numpy >= 1.24, used at environment/ants.py:83).  Nothing of the reference's source is
stored: a fixture holds only inputs (initial state, actions, the random draws
Walls.update consumed) and the outputs / state the reference produced.

Fixture layout (np.savez_compressed):
  meta_json        configuration (sizes, reward kind and weights, filter, max_time, ...)
  init_*           ants_xyt[N,3], seed[N], walls[W,H], food[W,H], anthill_xyr[3], rocks[R,4],
                   activation[N,C] (after the optional activate_all_pheromones call)
  ops[T]           0 = api.step, 1 = env.update, 2 = api.observation
  rot[T,N], ph[T,N], has_rot[T], has_ph[T]      actions of step ops
  jitter[T,N], hits[T]                          np.random.random draws of update ops
  after every op t:
    ants[T,N,3] prev[T,N,2] holding[T,N] mandibles[T,N] activation[T,N,C] reward_state[T,N]
    food[T,W,H] phero[T,C,W,H] explored[T,W,H] anthill_food[T] rock_centers[T,R,2] timestep[T]
  after step / observe ops:  obs[T,N,P,P,K] agent_state[T,N,2] reward[T,N] done[T]

Long runs (``grid_every``) thin the four big arrays: ``grids[T]`` marks the ops at which food, phero,
explored and obs were kept, and those arrays then hold one row per marked op, in op order (G rows
instead of T).  Everything else stays per op.  A file without ``grids`` keeps them at every op.

``place_ants`` / ``place_rocks`` set data on the reference's own objects after ``generate``: ant
positions anywhere on the grid (borders, corners, wall cells), rocks of any centre, radius and weight.
``init_*`` is recorded after them; such a file also carries wall_density / rich_food / placed_* in its
meta, so that a reader can tell which part of the initial state the generator's streams still explain.

The variant hooks (``variant_scenarios``) move the configuration off the values every earlier file shares: ``api_kw`` (the
five RLApi arguments), ``perception`` = (mask or None, shift[, radius]), ``delta`` (RL_api.DELTA, patched around the calls
that read it), ``reorder`` (the perceived list: objects dropped, repeated, in another order), ``max_hold``, ``max_val``
(None allowed), ``no_ph`` (rotation-only: activate_pheromone needs exactly two channels) and ``activation`` (the value
activate_all_pheromones sets).  Such a file's meta also holds delta, radius, perceived_arg (per perceived object: the
pheromone's index in ants.pheromones, else 0) and max_val = null for None; a mask of None is stored as an empty array.
"""
import json
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
sys.modules.setdefault("noise", types.ModuleType("noise"))  # food.py:2, anthill.py:2, utils.py:2
if not hasattr(np, "bool"):
    np.bool = bool  # ants.py:83
sys.path.insert(0, "/root/reference")

import environment.pheromone as ref_pheromone  # noqa: E402
import environment.RL_api as ref_rl_api  # noqa: E402
from environment.RL_api import RLApi  # noqa: E402
from environment.circle_obstacles import CircleObstacles  # noqa: E402
from environment.rewards.reward import Reward  # noqa: E402
from environment.rewards.reward_custom import ExplorationReward, All_Rewards, Food_Reward  # noqa: E402
from environment.pheromone import Pheromone  # noqa: E402
from environment.food import Food  # noqa: E402
from environment.walls import Walls  # noqa: E402
from environment.anthill import Anthill  # noqa: E402
from generator.environment_generator import EnvironmentGenerator  # noqa: E402
from generator.map_generators import CirclesGenerator  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
OP_STEP, OP_UPDATE, OP_OBSERVE = 0, 1, 2


class BernoulliWalls:
    """Stand-in for PerlinGenerator (needs the absent `noise` package): any bool[w,h] bitmap
    is a valid input to the path."""

    def __init__(self, density, rng):
        self.density, self.rng = density, rng

    def generate(self, w, h):
        return self.rng.random((w, h)) < self.density


class FoodNearAnthill:
    """CirclesGenerator plus one disc placed by the caller (to force pickups early and food
    lying on the anthill area at reset)."""

    def __init__(self, n, rmin, rmax, extra=None, rich=None):
        self.base = CirclesGenerator(n, rmin, rmax)
        self.extra = extra
        self.rich = rich  # optional rng: integer quantities 0..8 per cell instead of 0/1

    def generate(self, w, h):
        g = self.base.generate(w, h)
        if self.extra is not None:
            cx, cy, r = self.extra
            xs, ys = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
            g |= ((xs - cx) ** 2 + (ys - cy) ** 2) <= r * r
        if self.rich is not None:
            return g.astype(int) * self.rich.integers(1, 9, size=g.shape)
        return g


def make_reward(kind, weights):
    if kind == "exploration":
        return ExplorationReward()
    if kind == "food":
        return Food_Reward()
    if kind == "all":
        return All_Rewards(**weights)
    return Reward()


def run_scenario(name, *, w=64, h=64, n_ants=32, n_phero=2, steps=60, seed=3, wall_density=0.0,
                 n_rocks=0, reward="exploration", weights=None, float_activation=False,
                 filt=None, max_time=2000, script=None, food_extra=True, none_actions=False,
                 store_every=1, rich_food=False, place_ants=None, place_rocks=None, grid_every=None,
                 api_kw=None, perception=None, delta=None, reorder=None, max_hold=None, max_val=255, no_ph=False,
                 activation=10):
    rng = np.random.default_rng(1000 + seed)
    weights = weights or {}
    variant = (api_kw is not None or perception is not None or delta is not None or reorder is not None
               or max_hold is not None or max_val != 255 or no_ph or activation != 10)
    old_filter = ref_pheromone.DIFFUSE_FILTER
    old_delta = ref_rl_api.DELTA
    if filt is not None:
        ref_pheromone.DIFFUSE_FILTER = np.asarray(filt, dtype=float)  # read at call time, pheromone.py:44
    try:
        kw = dict(reward_threshold=1, max_speed=1, max_rot_speed=40 / 180 * np.pi, carry_speed_reduction=0.05,
                  backward_speed_reduction=0.5)
        kw.update(api_kw or {})
        api = RLApi(make_reward(reward, weights), **kw)
        # the generator draws the anthill from `random` first; peek so food can be put near it
        random.seed(seed)
        ax = int(random.random() * w * 0.5 + w * 0.25)
        ay = int(random.random() * h * 0.5 + h * 0.25)
        extra = (ax + 2, ay + 1, 6) if food_extra else None
        gen = EnvironmentGenerator(w, h, n_ants, n_phero, 0,
                                   FoodNearAnthill(6, 3, 6, extra, rng if rich_food else None),
                                   BernoulliWalls(wall_density, rng), max_time, seed=seed)
        if perception is not None and perception[0] is not None:
            gen.setup_perception(np.asarray(perception[0], dtype=bool), perception[1])
        if delta is not None:
            ref_rl_api.DELTA = delta  # read by RLApi.setup_perception at call time, RL_api.py:93
        env = gen.generate(api)
        if perception is not None and perception[0] is None:
            # generate() takes the radius from the mask's shape (environment_generator.py:102): no mask goes in afterwards
            api.setup_perception(perception[2], api.perceived_objects, None, perception[1])
        ref_rl_api.DELTA = old_delta
        ants = api.ants
        if max_hold is not None:
            ants.max_hold = max_hold
        for p in ants.pheromones:
            p.max_val = max_val
        rocks = None
        if place_ants is not None:
            # hook: positions anywhere on the grid.  Ants.__init__ (ants.py:27-30) and All_Rewards.setup
            # (reward_custom.py:77) have run on the generator's positions: redo what they derived from them.
            xyt = np.asarray(place_ants(rng, w, h, env), dtype=float)
            assert xyt.shape == (n_ants, 3)
            ants.ants[:] = xyt
            ants.warp_xy()
            ants.prev_ants = ants.ants.copy()
            if hasattr(api.reward, "previous_dist"):
                api.reward.previous_dist = api.reward.compute_distance(ants.x, ants.y)
        if n_rocks > 0 and place_rocks is not None:
            # hook: centres, radii and weights of the caller's choosing, float64 [n_rocks, 4]
            rk = np.asarray(place_rocks(rng, w, h, env), dtype=float)
            assert rk.shape == (n_rocks, 4)
            rocks = CircleObstacles(env, centers=rk[:, :2].copy(), radiuses=rk[:, 2].copy(), weights=rk[:, 3].copy())
            api.perceived_objects.append(rocks)
        elif n_rocks > 0:
            # generator's rock branch raises NameError (environment_generator.py:83-84):
            # build the object directly, near the anthill so ants collide with it.
            centers = np.stack([ax + rng.uniform(-12, 12, n_rocks), ay + rng.uniform(-12, 12, n_rocks)], 1)
            rocks = CircleObstacles(env, centers=centers.copy(), radiuses=rng.random(n_rocks) * 5 + 5,
                                    weights=rng.random(n_rocks) * 50 + 50)
            api.perceived_objects.append(rocks)
        if reorder is not None:
            api.perceived_objects = list(reorder(list(api.perceived_objects)))
        if float_activation:
            ants.activate_all_pheromones(np.ones((n_ants, n_phero)) * activation)  # collect_agent_memory.py:129-131

        objs = {type(o).__name__: o for o in env.objects}
        pheros = [o for o in env.objects if isinstance(o, Pheromone)]
        food, walls, anthill = objs["Food"], objs["Walls"], objs["Anthill"]
        kinds = []
        for o in api.perceived_objects:
            kinds.append(type(o).__name__)

        meta = dict(name=name, w=w, h=h, n_ants=n_ants, n_phero=n_phero, n_rocks=n_rocks,
                    reward=reward, weights=weights, max_time=max_time,
                    deposit_strength=256.0 if float_activation else 1.0,
                    filter=np.asarray(ref_pheromone.DIFFUSE_FILTER).tolist(),
                    perceived=kinds, fwd_delta=float(api.perception_fwd_delta),
                    max_speed=api.max_speed, max_rot_speed=api.max_rot_speed,
                    carry=api.carry_speed_reduction, backward=api.backward_speed_reduction,
                    max_hold=float(ants.max_hold), max_val=None if max_val is None else float(pheros[0].max_val),
                    reward_threshold=api.reward_threshold, seed=seed)
        if place_ants is not None or place_rocks is not None or grid_every is not None or variant:
            meta.update(wall_density=wall_density, rich_food=bool(rich_food), food_extra=bool(food_extra),
                        placed_ants=place_ants is not None, placed_rocks=place_rocks is not None)
        if variant:
            meta.update(delta=float(delta if delta is not None else old_delta), radius=int(api.perception_radius),
                        perceived_arg=[ants.pheromones.index(o) if isinstance(o, Pheromone) else 0
                                       for o in api.perceived_objects])
        rec = dict(
            init_ants_xyt=ants.ants.copy(), init_seed=ants.seed.copy(), init_walls=walls.map.copy(),
            init_food=food.qte.copy(), init_anthill_xyr=np.array([anthill.x, anthill.y, anthill.radius]),
            init_rocks=(np.concatenate([rocks.centers, rocks.radiuses[:, None], rocks.weights[:, None]], 1)
                        if rocks is not None else np.zeros((0, 4))),
            init_activation=ants.phero_activation.astype(float).copy(),
            init_anthill_area=anthill.area.copy(),
            mask=api.perception_mask.copy() if api.perception_mask is not None else np.zeros((0, 0), bool))

        if script is None:
            script = []
            for _ in range(steps):
                script += [OP_STEP, OP_UPDATE]
        T = len(script)
        # ops at which the grids and the observation are kept: both ops of every grid_every-th step and of the last
        grids = np.ones(T, bool) if grid_every is None else np.array(
            [(t % (2 * grid_every) in (0, 1)) or t >= T - 2 for t in range(T)])
        row = np.cumsum(grids) - 1  # op -> row of the thinned arrays
        G = int(grids.sum())
        P = api.perception_coords.shape[0]
        K = len(api.perceived_objects)
        R = n_rocks
        S = dict(ops=np.array(script, np.int8), rot=np.zeros((T, n_ants), np.int8),
                 ph=np.zeros((T, n_ants), np.int8), has_rot=np.zeros(T, np.uint8), has_ph=np.zeros(T, np.uint8),
                 jitter=np.zeros((T, n_ants)), hits=np.zeros(T, np.int32),
                 ants=np.zeros((T, n_ants, 3)), prev=np.zeros((T, n_ants, 2)), holding=np.zeros((T, n_ants)),
                 mandibles=np.zeros((T, n_ants), np.uint8), activation=np.zeros((T, n_ants, n_phero)),
                 reward_state=np.zeros((T, n_ants), np.uint8),
                 food=np.zeros((G, w, h), np.float32), phero=np.zeros((G, n_phero, w, h)),
                 explored=np.zeros((G, w, h), np.uint8), anthill_food=np.zeros(T),
                 rock_centers=np.zeros((T, R, 2)), timestep=np.zeros(T, np.int32),
                 obs=np.zeros((G, n_ants, P, P, K)), agent_state=np.zeros((T, n_ants, 2)),
                 reward=np.zeros((T, n_ants)), done=np.zeros(T, np.uint8), stored=np.zeros(T, np.uint8))
        if grid_every is not None:
            S["grids"] = grids.astype(np.uint8)
        real_random = np.random.random
        for t, op in enumerate(script):
            g = row[t] if grids[t] else None
            if op == OP_STEP:
                rot = rng.integers(-1, 2, n_ants)
                ph = rng.integers(0, 3, n_ants)
                use_rot, use_ph = True, True
                if none_actions:
                    use_rot, use_ph = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                if no_ph:
                    use_ph = False
                S["rot"][t], S["ph"][t] = rot, ph
                S["has_rot"][t], S["has_ph"][t] = use_rot, use_ph
                o, a, r, d = api.step(rot if use_rot else None, ph if use_ph else None)
                S["agent_state"][t], S["reward"][t], S["done"][t] = a, r, d
                if g is not None:
                    S["obs"][g] = o
            elif op == OP_OBSERVE:
                o, a, _ = api.observation()
                S["agent_state"][t] = a
                if g is not None:
                    S["obs"][g] = o
                S["reward"][t] = api.reward.rewards
            else:
                draws = []

                def recording_random(n=None):
                    v = real_random(n)
                    draws.append(np.atleast_1d(v).copy())
                    return v

                np.random.random = recording_random
                try:
                    env.update()
                finally:
                    np.random.random = real_random
                d = np.concatenate(draws) if draws else np.zeros(0)
                S["jitter"][t, : len(d)] = d
                S["hits"][t] = len(d)
            S["ants"][t] = ants.ants
            S["prev"][t] = ants.prev_ants[:, :2]
            S["holding"][t] = ants.holding
            S["mandibles"][t] = np.asarray(ants.mandibles).astype(np.uint8)
            S["activation"][t] = ants.phero_activation.astype(float)
            S["reward_state"][t] = np.asarray(ants.reward_state).astype(np.uint8)
            assert np.array_equal(food.qte.astype(np.float32).astype(np.float64), food.qte)
            if g is not None:
                S["food"][g] = food.qte
            store = ((t % (2 * store_every) in (0, 1)) or t >= T - 2) and g is not None
            S["stored"][t] = store
            if store:
                for c, p in enumerate(pheros):
                    S["phero"][g, c] = p.phero
            em = getattr(api.reward, "explored_map", None)
            if em is not None and g is not None:
                S["explored"][g] = em
            S["anthill_food"][t] = anthill.food
            if rocks is not None:
                S["rock_centers"][t] = rocks.centers
            S["timestep"][t] = env.timestep
        S["explored"] = np.packbits(S["explored"], axis=-1)
        path = os.path.join(OUT, name + ".npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, meta_json=np.array(json.dumps(meta)), **rec, **S)
        print("%-28s T=%3d  pickups(max holding)=%g  hits=%d  anthill_food=%g  %.0f KiB" % (
            name, T, S["holding"].max(), S["hits"].sum(), S["anthill_food"][-1], os.path.getsize(path) / 1024))
    finally:
        ref_pheromone.DIFFUSE_FILTER = old_filter
        ref_rl_api.DELTA = old_delta


def diffuse3(d, e=0.001):
    f = np.ones((3, 3)) * d
    f[1, 1] = 1 - 8 * d
    return f * (1 - e)


def radius3_filter(e=0.001):
    ax = np.arange(-3, 4)
    g = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2 * 1.5 ** 2))
    g[0, 1] *= 1.3  # deliberately asymmetric: pins convolution (flip) vs correlation
    g[5, 2] *= 0.7
    return g / g.sum() * (1 - e)


def ants_on_borders(rng, w, h, env):
    """A quarter of the ants in the four corner cells' neighbourhood, the rest within 1.5 cells of an edge, heading anywhere."""
    n = [o for o in env.objects if type(o).__name__ == "Ants"][0].n_ants
    xyt = np.zeros((n, 3))
    for i in range(n):
        d = rng.uniform(0.05, 1.5)
        if i % 4 == 0:  # a corner
            xyt[i, 0] = (0 if rng.integers(2) else w) + rng.uniform(-1.5, 1.5)
            xyt[i, 1] = (0 if rng.integers(2) else h) + rng.uniform(-1.5, 1.5)
        elif i % 2:     # left / right edge
            xyt[i, 0] = d if rng.integers(2) else w - d
            xyt[i, 1] = rng.uniform(0, h)
        else:           # bottom / top edge
            xyt[i, 0] = rng.uniform(0, w)
            xyt[i, 1] = d if rng.integers(2) else h - d
    xyt[:, 2] = rng.uniform(0, 2 * np.pi, n)
    return xyt  # (Ants.warp_xy folds the corner ants' negative coordinates)


def ants_spread(rng, w, h, env):
    """Uniform over the whole grid, wall cells included."""
    n = [o for o in env.objects if type(o).__name__ == "Ants"][0].n_ants
    return np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(0, 2 * np.pi, n)], 1)


def rocks_at(rows):
    """place_rocks hook from literal rows (cx, cy, radius, weight); cx / cy may be given as fractions of w / h."""
    def place(rng, w, h, env):
        rk = np.array(rows, dtype=float)
        rk[:, 0] *= w
        rk[:, 1] *= h
        return rk + np.concatenate([rng.uniform(-0.5, 0.5, (len(rk), 2)), np.zeros((len(rk), 2))], 1)
    return place


MAIN_WEIGHTS = dict(fct_explore=1, fct_food=2, fct_anthill=10, fct_explore_holding=1, fct_headinganthill=3)  # main.py:42

def crowd_scenarios():
    """Ants where the first 13 runs never put them: on the borders, on wall cells, under several rocks at once, many to a
    cell; rocks light enough to be pushed out of the grid.  tests/crowd_events.py counts what each run contains."""
    # c01: ants on the borders and in the corners, light rocks straddling the border
    run_scenario("c01_border_rocks", n_ants=48, steps=80, seed=21, wall_density=0.05, n_rocks=4,
                 place_ants=ants_on_borders, grid_every=8,
                 place_rocks=rocks_at([(0.0, 0.3, 6, 2.0), (0.98, 0.7, 5, 1.0), (0.5, 0.0, 7, 4.0), (0.02, 0.98, 4, 0.6)]))
    # c02: spread ants, dense walls, overlapping light rocks, float activation, All_Rewards
    run_scenario("c02_dense_walls_rocks", n_ants=64, steps=120, seed=22, wall_density=0.3, n_rocks=4, reward="all",
                 weights=MAIN_WEIGHTS, float_activation=True, place_ants=ants_spread, grid_every=15,
                 place_rocks=rocks_at([(0.3, 0.3, 8, 3.0), (0.4, 0.35, 7, 2.0), (0.7, 0.6, 9, 1.5), (0.6, 0.7, 6, 0.8)]))
    # c03: rocks under the 3 x 3 diffusion filter, on a grid that is no power of two
    run_scenario("c03_rocks_diffuse3x3", w=48, h=40, n_ants=40, steps=40, seed=23, wall_density=0.1, n_rocks=3,
                 filt=diffuse3(0.05), float_activation=True, place_ants=ants_spread, grid_every=5,
                 place_rocks=rocks_at([(0.3, 0.5, 6, 2.0), (0.45, 0.55, 5, 1.0), (0.8, 0.2, 5, 3.0)]))
    # c04: 64 ants on 16 x 12 cells (H no multiple of 8), two small light rocks
    run_scenario("c04_tiny_16x12", w=16, h=12, n_ants=64, steps=80, seed=34, wall_density=0.08, n_rocks=2, reward="all",
                 weights=MAIN_WEIGHTS, float_activation=True, food_extra=False, place_ants=ants_spread, grid_every=4,
                 place_rocks=rocks_at([(0.3, 0.4, 2.0, 0.5), (0.7, 0.6, 1.5, 0.2)]))
    # c05: rich food with rocks on top of it
    run_scenario("c05_rich_food_rocks", n_ants=48, steps=60, seed=25, wall_density=0.05, n_rocks=3, reward="all",
                 weights=MAIN_WEIGHTS, float_activation=True, rich_food=True, place_ants=ants_spread, grid_every=6,
                 place_rocks=rocks_at([(0.4, 0.4, 7, 2.0), (0.55, 0.5, 6, 1.0), (0.5, 0.65, 5, 0.6)]))
    # c06: 600 steps without rocks: scaled units and coordinates over a long horizon against the reference itself
    run_scenario("c06_long_600", n_ants=12, steps=600, seed=26, wall_density=0.1, reward="all", weights=MAIN_WEIGHTS,
                 float_activation=True, place_ants=ants_spread, grid_every=100)
    # oracle only (the device's drift over hundreds of rock pushes is DESIGN.md section 4's subject): 400 steps with rocks
    run_scenario("oracle_only/o01_rocks_400", n_ants=16, steps=400, seed=27, wall_density=0.1, n_rocks=3, reward="all",
                 weights=MAIN_WEIGHTS, float_activation=True, place_ants=ants_spread, grid_every=80,
                 place_rocks=rocks_at([(0.3, 0.3, 8, 3.0), (0.6, 0.6, 7, 1.0), (0.1, 0.8, 6, 0.5)]))


#: the generator's other mask (commented out at environment_generator.py:30-34): radius 2
MASK_5X5 = np.array([[0, 1, 1, 1, 0],
                     [1, 1, 1, 1, 1],
                     [1, 1, 1, 1, 1],
                     [0, 1, 1, 1, 0],
                     [0, 0, 1, 0, 0]], dtype=bool)
#: a 7 x 7 mask that is neither the default nor symmetric under any flip or transposition
MASK_7X7_OTHER = np.array([[0, 0, 0, 0, 0, 0, 1],
                           [0, 1, 1, 1, 1, 0, 0],
                           [1, 1, 1, 1, 1, 1, 0],
                           [1, 1, 1, 0, 1, 1, 1],
                           [0, 1, 1, 1, 1, 1, 1],
                           [0, 1, 1, 1, 1, 1, 0],
                           [1, 0, 1, 1, 0, 0, 0]], dtype=bool)
OTHER_WEIGHTS = dict(fct_explore=0.3, fct_food=7, fct_anthill=3, fct_explore_holding=0.7, fct_headinganthill=1.5)
NO_EXPLORE_WEIGHTS = dict(fct_explore=0, fct_food=2, fct_anthill=10, fct_explore_holding=0, fct_headinganthill=3)
DEG = np.pi / 180


def by_kind(order):
    """reorder hook: the perceived list rebuilt from kind names; "Pheromone0" / "Pheromone1" / ... name ants.pheromones[i]."""
    def pick(objs):
        pheros = [o for o in objs if isinstance(o, Pheromone)]
        named = {type(o).__name__: o for o in objs if not isinstance(o, Pheromone)}
        named.update({"Pheromone%d" % i: p for i, p in enumerate(pheros)})
        return [named[k] for k in order]
    return pick


def variant_scenarios():
    """Configurations no earlier recording has: every RLApi argument, both perception sizes and no mask, DELTA, the
    channel list, max_hold, max_val, 1 and 3 pheromones, other reward weights.  tests/test_variant_fixtures_cpu.py counts
    what each run contains."""
    # v01: carry 0.3 on rich food: an ant that holds 4 or 5 walks backwards, at half speed; another 7 x 7 mask on the
    # power-of-two grid (cell-meta path, fast k_perceive), shift 3, rocks
    run_scenario("v01_carry_backward", n_ants=32, steps=60, seed=41, wall_density=0.03, n_rocks=2, reward="all",
                 weights=MAIN_WEIGHTS, float_activation=True, rich_food=True, grid_every=5,
                 api_kw=dict(carry_speed_reduction=0.3), perception=(MASK_7X7_OTHER, 3))
    # v02: carry 0.5, backward 0.25, 25 degrees a step, rocks; a threshold (6) above the most an ant earns without a pickup
    # or a delivery: every one of the 49 sample points counts, masked or not (reward_custom.py:89), so a fresh window gives
    # 4.9, and heading for the anthill adds 0.3; a pickup of 3 or more (2 x taken) or a delivery (10) still passes it
    run_scenario("v02_backward_quarter", n_ants=32, steps=60, seed=42, wall_density=0.03, n_rocks=2, reward="all",
                 weights=MAIN_WEIGHTS, float_activation=True, rich_food=True, grid_every=5,
                 api_kw=dict(carry_speed_reduction=0.5, backward_speed_reduction=0.25, max_rot_speed=25 * DEG,
                             reward_threshold=6))
    # v03: 2.5 cells a step, 65 degrees, threshold 0.35, weights that are neither main.py's nor dyadic; rocks and walls
    run_scenario("v03_speed_threshold", n_ants=40, steps=50, seed=43, wall_density=0.05, n_rocks=3, reward="all",
                 weights=OTHER_WEIGHTS, float_activation=True, grid_every=5,
                 api_kw=dict(max_speed=2.5, max_rot_speed=65 * DEG, reward_threshold=0.35, carry_speed_reduction=0.12))
    # v04: All_Rewards that never counts explored cells (reward_custom.py:87), threshold 0.05
    run_scenario("v04_no_explore", n_ants=32, steps=60, seed=44, wall_density=0.03, reward="all",
                 weights=NO_EXPLORE_WEIGHTS, float_activation=True, grid_every=5, api_kw=dict(reward_threshold=0.05))
    # v05: the generator's 5 x 5 mask, no forward shift, rocks
    run_scenario("v05_mask5_shift0", n_ants=32, steps=50, seed=45, wall_density=0.05, n_rocks=2, grid_every=4,
                 perception=(MASK_5X5, 0))
    # v06: radius 5, no mask, shift 2.5, DELTA 1.37
    run_scenario("v06_radius5_delta", n_ants=24, steps=40, seed=47, wall_density=0.05, grid_every=8,
                 perception=(None, 2.5, 5), delta=1.37)
    # v07: Food before Anthill, both twice (RL_api.py:180-184 walks set, clear, set, clear: an ant over food on the anthill
    # area ends with open mandibles, where the generator's order closes them), pheromone 1 before pheromone 0, rocks;
    # max_hold 2 on rich food.  Every op keeps its grids: the test reads the food under every pickup.
    run_scenario("v07_reordered_hold2", n_ants=32, steps=60, seed=48, wall_density=0.03, n_rocks=2, reward="all",
                 weights=MAIN_WEIGHTS, float_activation=True, rich_food=True, max_hold=2,
                 reorder=by_kind(["Food", "Anthill", "Pheromone1", "Ants", "Food", "Pheromone0", "Walls", "CircleObstacles",
                                  "Anthill"]))
    # v08: neither Food nor a pheromone perceived (no ant can pick anything up), Pheromone(max_val=None): deposits unclipped
    run_scenario("v08_no_food_no_phero", n_ants=32, steps=50, seed=49, wall_density=0.05, float_activation=True,
                 grid_every=5, max_val=None, reorder=by_kind(["Ants", "Anthill", "Walls"]))
    # v09: Food but no Anthill (mandibles close and never open), ExplorationReward with other motion parameters
    run_scenario("v09_food_no_anthill", n_ants=32, steps=50, seed=50, wall_density=0.03, rich_food=True, grid_every=5,
                 api_kw=dict(max_speed=1.75, max_rot_speed=90 * DEG, carry_speed_reduction=0.12, backward_speed_reduction=0.75),
                 reorder=by_kind(["Ants", "Pheromone0", "Pheromone1", "Walls", "Food"]))
    # v10: one pheromone with max_val 100, deposits of 60 (two ants to a cell reach the cap); Food_Reward, other motion
    run_scenario("v10_one_phero_max100", n_ants=48, n_phero=1, steps=60, seed=51, wall_density=0.03, reward="food",
                 float_activation=True, activation=60, no_ph=True, max_val=100, grid_every=5,
                 api_kw=dict(max_speed=1.5, max_rot_speed=55 * DEG, carry_speed_reduction=0.1))
    # v11: three pheromones under a random 11 x 11 mask
    run_scenario("v11_three_phero_mask11", n_ants=24, n_phero=3, steps=40, seed=52, wall_density=0.05,
                 float_activation=True, no_ph=True, grid_every=10, store_every=2,
                 perception=(np.random.default_rng(52).random((11, 11)) < 0.7, 4))


if __name__ == "__main__":
    run_scenario("s01_plain", steps=60, seed=3)
    run_scenario("s02_walls", steps=60, seed=4, wall_density=0.05)
    run_scenario("s03_walls_rocks", steps=60, seed=5, wall_density=0.05, n_rocks=3)
    run_scenario("s04_float_activation", steps=60, seed=6, wall_density=0.05, float_activation=True)
    run_scenario("s05_all_rewards", steps=60, seed=7, wall_density=0.05, reward="all", weights=MAIN_WEIGHTS,
                 float_activation=True)
    run_scenario("s06_food_reward", steps=40, seed=8, wall_density=0.03, reward="food")
    run_scenario("s07_diffuse3x3", steps=40, seed=9, wall_density=0.05, filt=diffuse3(0.05), float_activation=True)
    run_scenario("s08_radius3", steps=30, seed=10, wall_density=0.05, filt=radius3_filter(), float_activation=True)
    # odd call patterns: observation() before the first step (main.py:88), two steps without an
    # update, None actions (RL_api.py:187,190), `done` at timestep == max_time (RL_api.py:200)
    scr = [OP_OBSERVE] + [OP_STEP, OP_UPDATE] * 4 + [OP_STEP, OP_STEP, OP_UPDATE, OP_OBSERVE, OP_UPDATE] + \
          [OP_STEP, OP_UPDATE] * 10
    run_scenario("s09_script_none_done", seed=11, wall_density=0.05, n_rocks=2, reward="all",
                 weights=MAIN_WEIGHTS, max_time=9, script=scr, none_actions=True)
    run_scenario("s10_rect_96x48", w=96, h=48, n_ants=40, steps=40, seed=12, wall_density=0.05, n_rocks=2)
    run_scenario("s11_base_reward", steps=12, seed=13, wall_density=0.05, reward="none")
    run_scenario("s13_rich_food", steps=50, seed=15, wall_density=0.03, reward="all", weights=MAIN_WEIGHTS,
                 float_activation=True, rich_food=True)
    run_scenario("s12_256_n256", w=256, h=256, n_ants=256, steps=20, seed=14, wall_density=0.05,
                 n_rocks=4, store_every=5)
    crowd_scenarios()
    variant_scenarios()
