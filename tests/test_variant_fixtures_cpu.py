"""Certifies, from their arrays alone, that the variant fixtures (tests/golden/v*.npz, make_golden.variant_scenarios)
contain what they were recorded for: every configuration the earlier recordings share is moved off its value in at least
one of them, and the code that only such a value reaches (the backward move, a threshold other than 1, All_Rewards without
exploration, a pickup capped below 5, the mandible walk in another order) runs often enough in the reference's own run
to be pinned by it.  No file is large, no coordinate sits where a last-ulp difference flips a cell, and a one-ulp change
of the initial state stays a hundred times below the GPU's coordinate tolerance, in the recordings and in the oracle runs
that tests/test_gpu_crowd_deferred.py compares the device with."""
import os

import numpy as np
import pytest

import crowd_events as ce
from helpers import GOLDEN, OP_STEP, crowd_fixture_names, load_fixture, variant_fixture_names
from test_crowd_fixtures_cpu import ENV_ID_BASE, MAX_BYTES, MIN_DISTANCE_TO_INTEGER, N_ENVS, SENSITIVITY_BOUND, _largest_difference

from antsrl_amd import config as cm

MAX_BYTES_TOGETHER = 5_000_000
DEG = np.pi / 180
DEFAULT_ORDER = ["Ants", "Pheromone", "Pheromone", "Anthill", "Walls", "Food"]
MAIN_WEIGHTS = dict(fct_explore=1, fct_food=2, fct_anthill=10, fct_explore_holding=1, fct_headinganthill=3)

#: event -> the count at least one recording must reach (the issue's floors)
FLOORS = {"backward_ant_steps": 200, "capped_pickups": 10, "moves_over_two_cells": 1, "food_reward_drops": 5}
#: ant-steps whose reward lies strictly between the file's threshold and 1, for every file with a threshold below 1
FLOOR_BETWEEN_THRESHOLD_AND_ONE = 50
#: a threshold above 1 shows only where a reward lies in (1, threshold] (lit at the default threshold, dark here) and is
#: told from "never lit" only where some reward exceeds it.  Floors set like the one above: 50 of the first, and as many
#: of the second as the Food_Reward drops (5), both two orders below the 1920 ant-steps of such a file.  "Above the
#: largest exploration reward" is judged on what an ant can earn without a pickup or a delivery: every sample point of a
#: fresh window counts, masked or not (reward_custom.py:89), times the larger explore weight, plus the heading term.
FLOOR_BETWEEN_ONE_AND_THRESHOLD, FLOOR_ABOVE_HIGH_THRESHOLD = 50, 5

NAMES = variant_fixture_names()


def is_backward_file(meta):
    """Ants that hold max_hold walk backwards: holding * carry > 1 is reachable."""
    return meta["max_hold"] * meta["carry"] > 1


def count_events(F, meta, init):
    steps = np.nonzero(F["ops"] == OP_STEP)[0]
    size = np.array([meta["w"], meta["h"]], float)
    n = dict.fromkeys(FLOORS, 0)
    n.update(between_threshold_and_one=0, between_one_and_threshold=0, above_threshold=0, reward_state_lit=0,
             lit_with_holding_unchanged=0)
    thr = meta["reward_threshold"]
    before_xy, before_prev, before_hold = F["init_ants_xyt"][:, :2], F["init_ants_xyt"][:, :2], np.zeros(meta["n_ants"])
    food_before, food_known = F["init_food"].astype(np.float64), True
    for t, op in enumerate(F["ops"]):
        if op == OP_STEP:
            hold, rew = F["holding"][t], F["reward"][t]
            # RL_api.py:194-195: the move of this step uses the holding its own mandible update left
            n["backward_ant_steps"] += int((hold * meta["carry"] > 1).sum())
            d = np.abs(F["ants"][t][:, :2] - before_xy)
            d = np.minimum(d, size - d)  # (np.mod folds a move across the edge)
            n["moves_over_two_cells"] += int((np.sqrt((d ** 2).sum(1)) > 2).sum())
            n["between_threshold_and_one"] += int(((rew > thr) & (rew < 1)).sum())
            n["between_one_and_threshold"] += int(((rew > 1) & (rew <= thr)).sum())
            n["above_threshold"] += int((rew > thr).sum())
            # (255 right after a step: lit by this step; an earlier 255 has decayed to 229 at most, ants.py:130)
            n["lit_with_holding_unchanged"] += int(((F["reward_state"][t] == 255) & (hold == before_hold)).sum())
            if meta["reward"] == "food":
                n["food_reward_drops"] += int(((hold < before_hold) & (rew == 10)).sum())
            if food_known:
                # ants.py:111: taken = min(max_hold, food under the ant's previous position); counted where the file
                # kept the food grid of the op before
                cell = before_prev.astype(int)
                under = food_before[cell[:, 0], cell[:, 1]]
                n["capped_pickups"] += int(((hold > before_hold) & (under > meta["max_hold"]) & (meta["max_hold"] < 5)).sum())
        n["reward_state_lit"] += int((F["reward_state"][t] == 255).sum())
        before_xy, before_prev, before_hold = F["ants"][t][:, :2], F["prev"][t], F["holding"][t]
        food_known = bool(F["grids"][t])
        if food_known:
            food_before = F["food"][F["grid_row"][t]].astype(np.float64)
    return n


@pytest.fixture(scope="module")
def loaded():
    return {name: load_fixture(name) for name in NAMES}


@pytest.fixture(scope="module")
def counted(loaded):
    out = {name: count_events(F, meta, init) for name, (cfg, init, F, meta) in loaded.items()}
    for name, c in out.items():
        print(name, c)
    return out


@pytest.fixture(scope="module")
def deferred_runs(loaded):
    """name -> (per-env trajectories, the same from the nudged start) of the oracle driven as the deferred GPU test drives."""
    out = {}
    for name in NAMES:
        cfg, init, F, meta = load_fixture(name, N_ENVS)
        out[name] = (ce.oracle_deferred_run(cfg, init, F, meta, ENV_ID_BASE)[0],
                     ce.oracle_deferred_run(cfg, init, F, meta, ENV_ID_BASE, nudge=True)[0])
    return out


def test_the_names_keep_clear_of_the_crowd_files():
    assert 9 <= len(NAMES) <= 11 and not set(NAMES) & set(crowd_fixture_names())


def test_the_issue_s_configurations_are_there(loaded):
    M = {n: m for n, (_, _, _, m) in loaded.items()}
    F = {n: f for n, (_, _, f, _) in loaded.items()}
    for m in M.values():
        assert {"delta", "radius", "perceived_arg", "wall_density", "rich_food", "food_extra"} <= set(m)

    def some(pred):
        return any(pred(M[n], F[n]) for n in NAMES)

    def weights(m):
        return {k: float(v) for k, v in (m["weights"] or {}).items()}

    def most_without_food(m, f):
        """The largest All_Rewards reward of an ant that neither picks up nor delivers: a fresh window + the heading term."""
        w, points = weights(m), (2 * m["radius"] + 1) ** 2
        return points / 10 * max(w["fct_explore"], w["fct_explore_holding"]) + 0.1 * w["fct_headinganthill"]

    # a: backward motion, at 0.5 and at another factor
    assert some(lambda m, f: m["carry"] >= 0.3 and m["rich_food"] and m["reward"] == "all" and m["backward"] == 0.5)
    assert some(lambda m, f: m["carry"] >= 0.3 and m["rich_food"] and m["reward"] == "all" and m["backward"] not in (0.5, 1))
    # b: speed, rotation, thresholds, weights
    assert some(lambda m, f: m["max_speed"] == 2.5 and abs(m["max_rot_speed"] - 40 * DEG) > 1e-3 and m["n_rocks"] and m["wall_density"] > 0)
    assert some(lambda m, f: m["reward_threshold"] < 1)
    assert some(lambda m, f: m["reward"] == "all" and m["reward_threshold"] > most_without_food(m, f))
    assert some(lambda m, f: m["reward"] == "all" and weights(m) != MAIN_WEIGHTS
                and any(v * 8 != int(v * 8) for v in weights(m).values()) and 7 in weights(m).values()
                and weights(m)["fct_explore_holding"] != weights(m)["fct_explore"])
    # c: All_Rewards that counts no explored cell
    assert some(lambda m, f: m["reward"] == "all" and weights(m)["fct_explore"] == 0 and weights(m)["fct_explore_holding"] == 0)
    # d: the 5 x 5 mask without a shift, with rocks; another 7 x 7 mask on a power-of-two grid
    assert some(lambda m, f: m["radius"] == 2 and f["mask"].shape == (5, 5) and m["fwd_delta"] == 0 and m["n_rocks"])
    assert some(lambda m, f: m["radius"] == 3 and f["mask"].shape == (7, 7) and not np.array_equal(f["mask"], cm.DEFAULT_MASK)
                and not (m["w"] & (m["w"] - 1)) and not (m["h"] & (m["h"] - 1)))
    # e: radius 5, no mask, shift 2.5, DELTA 1.37
    assert some(lambda m, f: m["radius"] == 5 and f["mask"].size == 0 and m["fwd_delta"] == 2.5 and m["delta"] == 1.37)
    # f: Food before Anthill, Food twice, pheromone 1 before pheromone 0, rocks; max_hold below 5 on rich food
    assert some(lambda m, f: m["perceived"].index("Food") < m["perceived"].index("Anthill") and m["perceived"].count("Food") == 2
                and [a for k, a in zip(m["perceived"], m["perceived_arg"]) if k == "Pheromone"] == [1, 0] and m["n_rocks"])
    assert some(lambda m, f: m["max_hold"] in (2, 2.5) and m["rich_food"])
    # g: neither Food nor a pheromone perceived and max_val None; Anthill without Food; Food without Anthill
    assert some(lambda m, f: "Food" not in m["perceived"] and "Pheromone" not in m["perceived"] and m["max_val"] is None
                and f["holding"].max() == 0)
    assert some(lambda m, f: "Anthill" in m["perceived"] and "Food" not in m["perceived"])
    assert some(lambda m, f: "Food" in m["perceived"] and "Anthill" not in m["perceived"] and f["holding"].max() > 0)
    # h: one pheromone capped at 100; three pheromones under an 11 x 11 mask; rotation only, float activation
    assert some(lambda m, f: m["n_phero"] == 1 and m["max_val"] == 100 and not f["has_ph"].any() and m["deposit_strength"] != 1.0
                and f["phero"].max() == 100)
    assert some(lambda m, f: m["n_phero"] == 3 and f["mask"].shape == (11, 11) and not f["mask"].all() and not f["has_ph"].any()
                and m["deposit_strength"] != 1.0)
    # i: Food_Reward and ExplorationReward with other motion parameters
    for kind in ("food", "exploration"):
        assert some(lambda m, f: m["reward"] == kind and m["max_speed"] != 1 and m["carry"] != 0.05
                    and abs(m["max_rot_speed"] - 40 * DEG) > 1e-3)
    # and the perceived lists are not all the generator's
    assert some(lambda m, f: m["perceived"][:6] != DEFAULT_ORDER)


@pytest.mark.parametrize("event", sorted(FLOORS))
def test_event_floor(counted, event):
    counts = {name: c[event] for name, c in counted.items()}
    print(event, counts)
    assert max(counts.values()) >= FLOORS[event], counts


def test_backward_motion_at_both_factors(loaded, counted):
    """>= 200 backward ant-steps in a file with backward_speed_reduction 0.5 and in one with another factor."""
    half = {n: counted[n]["backward_ant_steps"] for n in NAMES if loaded[n][3]["backward"] == 0.5}
    other = {n: counted[n]["backward_ant_steps"] for n in NAMES if loaded[n][3]["backward"] not in (0.5, 1)}
    print(half, other)
    assert max(half.values()) >= FLOORS["backward_ant_steps"] and max(other.values()) >= FLOORS["backward_ant_steps"]


def test_rewards_on_both_sides_of_every_threshold(loaded, counted):
    seen_low = seen_high = False
    for name in NAMES:
        thr, c = loaded[name][3]["reward_threshold"], counted[name]
        print(name, "threshold", thr, {k: c[k] for k in ("between_threshold_and_one", "between_one_and_threshold",
                                                         "above_threshold", "reward_state_lit", "lit_with_holding_unchanged")})
        if thr < 1:
            seen_low = True
            assert c["between_threshold_and_one"] >= FLOOR_BETWEEN_THRESHOLD_AND_ONE, name
        elif thr > 1:
            seen_high = True
            assert c["between_one_and_threshold"] >= FLOOR_BETWEEN_ONE_AND_THRESHOLD, name
            assert c["above_threshold"] >= FLOOR_ABOVE_HIGH_THRESHOLD, name
            # ... and on the recording itself: exploration and heading alone never light the state
            assert c["lit_with_holding_unchanged"] == 0, name
        # ants.py:119-121 on the recording itself: the state is lit exactly where a reward passed the threshold
        assert (c["reward_state_lit"] > 0) == (c["above_threshold"] > 0), name
    assert seen_low and seen_high


def test_no_explored_cell_without_explore_weights(loaded):
    hit = 0
    for name in NAMES:
        cfg, init, F, meta = loaded[name]
        w = meta["weights"] or {}
        if meta["reward"] == "all" and w["fct_explore"] == 0 and w["fct_explore_holding"] == 0:
            assert not F["explored"].any(), name
            assert (F["reward"] > 0).any(), name
            hit += 1
    assert hit


def test_the_mandible_order_shows(loaded):
    """The oracle replays the recording whose list puts Food before Anthill with the two kinds swapped (the generator's
    order): somewhere the mandibles must differ from the recorded ones, or the recording would not tell the orders apart."""
    from oracle.oracle import Oracle
    hit = 0
    for name in NAMES:
        cfg, init, F, meta = loaded[name]
        per = meta["perceived"]
        if not ("Food" in per and "Anthill" in per and per.index("Food") < per.index("Anthill")):
            continue
        swapped = cfg.copy()
        for k in range(cfg.n_channels):
            if cfg.channel_kind[k] in (cm.CH_FOOD, cm.CH_ANTHILL):
                swapped.channel_kind[k] = cm.CH_FOOD + cm.CH_ANTHILL - cfg.channel_kind[k]
        differ = 0
        for c, must_match in ((cfg, True), (swapped, False)):
            o = Oracle(c, init)
            if meta["deposit_strength"] != 1.0:
                o.set_activation(np.broadcast_to(F["init_activation"], o.activation.shape))
            for t, op in enumerate(F["ops"]):
                if op == OP_STEP:
                    o.step(F["rot"][t][None] if F["has_rot"][t] else None, F["ph"][t][None] if F["has_ph"][t] else None, want_obs=False)
                elif op == ce.OP_OBSERVE:
                    o.observe(want_obs=False)
                else:
                    o.update(F["jitter"][t][None])
                if must_match:
                    np.testing.assert_array_equal(o.mandibles[0], F["mandibles"][t])
                else:
                    differ += int((o.mandibles[0] != F["mandibles"][t]).sum())
        print(name, "mandibles that differ under the generator's order:", differ)
        assert differ > 0, name
        hit += 1
    assert hit


@pytest.mark.parametrize("name", NAMES)
def test_size(name):
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= MAX_BYTES


def test_size_together():
    total = sum(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) for n in NAMES)
    print(total)
    assert total <= MAX_BYTES_TOGETHER


@pytest.mark.parametrize("name", NAMES)
def test_no_coordinate_next_to_an_integer(loaded, name):
    cfg, init, F, meta = loaded[name]
    d = ce.min_distance_to_integer(ce.from_fixture(F, meta, init))
    print(name, d)
    assert d >= MIN_DISTANCE_TO_INTEGER


@pytest.mark.parametrize("name", NAMES)
def test_no_coordinate_next_to_an_integer_in_the_deferred_runs(deferred_runs, name):
    d = min(ce.min_distance_to_integer(tr) for tr in deferred_runs[name][0])
    print(name, d)
    assert d >= MIN_DISTANCE_TO_INTEGER


@pytest.mark.parametrize("name", NAMES)
def test_one_ulp_sensitivity_of_the_replay(loaded, name):
    cfg, init, F, meta = loaded[name]
    first = ce.oracle_replay_coordinates(cfg, init, F, meta)
    np.testing.assert_array_equal(first[0], F["ants"])
    d = _largest_difference(first, ce.oracle_replay_coordinates(cfg, init, F, meta, nudge=True))
    print(name, d)
    assert d <= SENSITIVITY_BOUND


@pytest.mark.parametrize("name", NAMES)
def test_one_ulp_sensitivity_of_the_deferred_runs(deferred_runs, name):
    d = max(_largest_difference((a["ants"], a["rock_centers"]), (b["ants"], b["rock_centers"]))
            for a, b in zip(*deferred_runs[name]))
    print(name, d)
    assert d <= SENSITIVITY_BOUND


def test_the_deferred_runs_hold_the_backward_move_and_the_threshold():
    """What tests/test_gpu_crowd_deferred.py relies on: the oracle's deferred runs of the backward files and of the files with
    another threshold still contain their events (the library's own wall jitter, not the recorded one)."""
    for name in NAMES:
        cfg, init, F, meta = load_fixture(name, N_ENVS)
        thr = meta["reward_threshold"]
        if not (is_backward_file(meta) or thr != 1):
            continue
        trs, outs, orc = ce.oracle_deferred_run(cfg, init, F, meta, ENV_ID_BASE)
        rew = np.stack([o[2] for o in outs])  # [steps, E, N]
        hold = np.stack([o[1][..., 0] for o in outs])
        back = int((hold * meta["carry"] > 1).sum())
        between = int(((rew > thr) & (rew < 1)).sum()) if thr < 1 else int(((rew > 1) & (rew <= thr)).sum())
        print(name, "deferred: backward ant-steps", back, "rewards between the threshold and 1 / 1 and the threshold", between)
        if is_backward_file(meta):
            assert back >= FLOORS["backward_ant_steps"], name
        if thr != 1:
            assert between >= FLOOR_BETWEEN_THRESHOLD_AND_ONE, name
