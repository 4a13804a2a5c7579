#!/usr/bin/env python3
"""Generates tests/golden/contract/custom_reward_ref.npz by RUNNING THE REFERENCE — build container only (the reference
lives at /root/reference there and never travels):

    python tests/golden/make_custom_reward_golden.py

What it pins: the reference's extension point for rewards.  RLApi hands a caller's Reward subclass the integer cells
every ant perceives (Reward.observation, RL_api.py:164), takes the reward from Reward.step (RL_api.py:202) and flashes the
ants with Ants.give_reward(reward - reward_threshold) (RL_api.py:203, ants.py:119-121), which Ants.update then decays
(ants.py:130).  The probe of tests/custom_reward_probe.py (the same file the tests replay here) runs on the reference in two
cases, each 32 x 24 cells with 12 ants that start within 4 cells of the four borders, walls, food, the initial
observation() call and 25 x (api.step, env.update):

    mask   the default 7 x 7 mask, shift 4, reward_threshold 0.3, two pheromones
    open   radius 2 without a mask, shift 0, reward_threshold -0.05, two pheromones (Ants.activate_pheromone takes two)

Stored per case: the init arrays, the actions, the wall jitter, every obs_coords the probe was handed (int16; [0] is the
initial observation's), the two other things its reward rests on (which unmasked cells showed food, bit-packed along the
last axis, and which ants held food), every reward RLApi.step returned, the probe's rewards after the initial observation, and
reward_state after each step and after each update.  Same import shims as make_phase_golden.py; only inputs and recorded
outputs are stored."""
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
sys.modules.setdefault("noise", types.ModuleType("noise"))
if not hasattr(np, "bool"):
    np.bool = bool
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from environment.RL_api import RLApi  # noqa: E402
from environment.rewards.reward import Reward  # noqa: E402
from generator.environment_generator import EnvironmentGenerator  # noqa: E402
from custom_reward_probe import make_probe  # noqa: E402
from make_golden import BernoulliWalls, FoodNearAnthill  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "contract")
W, H, N, STEPS = 32, 24, 12, 25


def near_borders(rng, w, h, n):
    """Ant i within 4 cells of border i % 4 (x = 0, x = w, y = 0, y = h), anywhere along it, heading anywhere."""
    xyt = np.zeros((n, 3))
    for i in range(n):
        d = rng.uniform(0.05, 3.95)
        along = rng.uniform(0, 1)
        xyt[i, :2] = [(d, along * h), (w - d, along * h), (along * w, d), (along * w, h - d)][i % 4]
        xyt[i, 2] = rng.uniform(0, 2 * np.pi)
    return xyt


def run(tag, seed, threshold, n_phero, masked):
    rng = np.random.default_rng(4000 + seed)
    probe = make_probe(Reward)()
    api = RLApi(probe, reward_threshold=threshold, max_speed=1, max_rot_speed=40 / 180 * np.pi, carry_speed_reduction=0.05,
                backward_speed_reduction=0.5)
    random.seed(seed)
    ax = int(random.random() * W * 0.5 + W * 0.25)
    ay = int(random.random() * H * 0.5 + H * 0.25)
    gen = EnvironmentGenerator(W, H, N, n_phero, 0, FoodNearAnthill(5, 2, 4, (ax + 2, ay + 1, 3), None), BernoulliWalls(0.06, rng),
                               2000, seed=seed)
    env = gen.generate(api)
    if not masked:  # (generate() takes the radius from the mask's shape, environment_generator.py:102: no mask goes in afterwards)
        api.setup_perception(2, api.perceived_objects, None, 0)
    ants = api.ants
    ants.ants[:] = near_borders(rng, W, H, N)
    ants.warp_xy()
    ants.prev_ants = ants.ants.copy()
    objs = {type(o).__name__: o for o in env.objects}
    food, walls, anthill = objs["Food"], objs["Walls"], objs["Anthill"]
    rec = {"init_ants_xyt": ants.ants.copy(), "init_seed": ants.seed.copy(), "init_walls": walls.map.copy(),
           "init_food": food.qte.copy(), "init_anthill_xyr": np.array([anthill.x, anthill.y, anthill.radius]),
           "mask": api.perception_mask.copy() if masked else np.zeros((0, 0), bool),
           "radius": np.array(api.perception_radius), "shift": np.array(float(api.perception_fwd_delta)),
           "threshold": np.array(float(threshold)), "n_phero": np.array(n_phero)}
    rot = rng.integers(-1, 2, (STEPS, N))
    ph = rng.integers(0, 3, (STEPS, N))
    jit = np.zeros((STEPS, N))
    api.observation()
    rec["reward_observation0"] = np.asarray(probe.rewards, dtype=float).copy()
    rewards, rs_step, rs_update = [], [], []
    real_random = np.random.random
    for t in range(STEPS):
        _, _, reward, _ = api.step(rot[t], ph[t])
        rewards.append(np.asarray(reward, dtype=float).copy())
        rs_step.append(np.asarray(ants.reward_state).astype(np.uint8))
        draws = []

        def recording(n=None):
            v = real_random(n)
            draws.append(np.atleast_1d(v).copy())
            return v
        np.random.random = recording
        try:
            env.update()
        finally:
            np.random.random = real_random
        d = np.concatenate(draws) if draws else np.zeros(0)
        jit[t, :len(d)] = d
        rs_update.append(np.asarray(ants.reward_state).astype(np.uint8))
    coords = np.stack(probe.seen_coords)
    assert coords.shape == (STEPS + 1, N, 2 * api.perception_radius + 1, 2 * api.perception_radius + 1, 2) and coords.max() < 2 ** 15
    rec.update(food_seen=np.packbits(np.stack(probe.seen_food), axis=-1), holding_seen=np.stack(probe.seen_holding),
               rot=rot.astype(np.int8), ph=ph.astype(np.int8), jitter=jit, obs_coords=coords.astype(np.int16),
               rewards=np.stack(rewards), reward_state_step=np.stack(rs_step), reward_state_update=np.stack(rs_update))
    r = rec["rewards"]
    print("%-5s rewards %.3f .. %.3f, above the threshold %d of %d, wall hits %d, flashed ants after the steps %d" % (
        tag, r.min(), r.max(), int((r - threshold > 0).sum()), r.size, int((jit != 0).sum()), int((rec["reward_state_step"] == 255).sum())))
    return {"%s_%s" % (tag, k): v for k, v in rec.items()}


if __name__ == "__main__":
    out = {}
    out.update(run("mask", 31, 0.3, 2, True))
    out.update(run("open", 32, -0.05, 2, False))
    path = os.path.join(OUT, "custom_reward_ref.npz")
    np.savez_compressed(path, **out)
    print("%s  %.0f KiB" % (path, os.path.getsize(path) / 1024))
