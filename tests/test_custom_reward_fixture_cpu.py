"""tests/golden/contract/custom_reward_ref.npz (tests/golden/make_custom_reward_golden.py: the reference itself under the probe
of tests/custom_reward_probe.py) holds what it is for — counted from its own arrays, as tests/crowd_events.py does for the
crowd fixtures.  Conditions on the fixture, not measurements of the code under test:

  * perception patches wrap over each of the four borders (the toroidal wrap of obs_coords is exercised on every side);
  * `open` (reward_threshold -0.05) holds rewards BELOW the negative threshold — a handle that gave its own reward of 0
    against that threshold would flash those ants — and rewards of exactly 0, which are above it and do flash;
  * `mask` (reward_threshold 0.3) holds rewards on both sides of the threshold;
  * the stored reward_state is what Ants.give_reward / Ants.update make of the stored rewards (ants.py:119-121, :130);
  * the probe, replayed with numpy on the stored coordinates, returns the stored rewards: the coordinates are the ones the
    reference's rewards were computed from."""
import os

import numpy as np
import pytest

from custom_reward_probe import probe_reward
from helpers import GOLDEN

CASES = ("mask", "open")
W, H = 32, 24


@pytest.fixture(scope="module")
def F():
    return dict(np.load(os.path.join(GOLDEN, "contract", "custom_reward_ref.npz")))


def case(F, tag):
    return {k[len(tag) + 1:]: v for k, v in F.items() if k.startswith(tag + "_")}


@pytest.mark.parametrize("tag", CASES)
def test_shapes_and_ranges(F, tag):
    g = case(F, tag)
    T, N = g["rot"].shape
    P = 2 * int(g["radius"]) + 1
    assert (T, N) == (25, 12) and g["init_walls"].shape == (W, H) and g["init_walls"].any() and (g["init_food"] > 0).any()
    assert g["obs_coords"].shape == (T + 1, N, P, P, 2) and g["obs_coords"].dtype == np.int16
    c = g["obs_coords"]
    assert c.min() >= 0 and c[..., 0].max() < W and c[..., 1].max() < H
    assert g["rewards"].shape == g["reward_state_step"].shape == g["reward_state_update"].shape == (T, N)
    xy = g["init_ants_xyt"][:, :2]
    d = np.minimum.reduce([xy[:, 0], W - xy[:, 0], xy[:, 1], H - xy[:, 1]])
    assert (d < 4).all(), "every ant starts within 4 cells of a border"
    assert (g["mask"].shape == (P, P)) == (tag == "mask")


@pytest.mark.parametrize("tag", CASES)
def test_patches_wrap_over_each_of_the_four_borders(F, tag):
    c = case(F, tag)["obs_coords"].astype(np.int64)
    P = c.shape[2]
    centre = c[:, :, P // 2, P // 2]
    x, y = c[..., 0].reshape(c.shape[:2] + (-1,)), c[..., 1].reshape(c.shape[:2] + (-1,))
    # a patch whose centre lies in the low half and that holds a cell within P of the far edge has wrapped below 0 (a cell
    # lies at most rint(1.1 * sqrt(2) * r + 0.5) = 5 cells from the centre at r = 3: on the smaller side, h = 24, an unwrapped
    # patch centred at 11 or below ends at 16 < 17 = h - P); likewise above the far edge
    wraps = {"x < 0": (centre[..., 0] < W // 2) & (x.max(-1) >= W - P), "x >= w": (centre[..., 0] >= W // 2) & (x.min(-1) < P),
             "y < 0": (centre[..., 1] < H // 2) & (y.max(-1) >= H - P), "y >= h": (centre[..., 1] >= H // 2) & (y.min(-1) < P)}
    for border, hit in wraps.items():
        assert int(hit.sum()) >= 1, "%s: no patch wraps over %s" % (tag, border)


def test_open_holds_rewards_below_its_negative_threshold_and_zeros_above_it(F):
    g = case(F, "open")
    thr = float(g["threshold"])
    assert thr == -0.05
    r = g["rewards"]
    assert int((r < thr).sum()) >= 1, "no reward below the negative threshold: a reward of 0 given by the handle would not be told apart"
    assert int((r == 0).sum()) >= 1, "no reward of exactly 0 (above the negative threshold: it flashes)"


def test_mask_holds_rewards_on_both_sides_of_its_threshold(F):
    g = case(F, "mask")
    thr = float(g["threshold"])
    assert thr == 0.3
    assert int((g["rewards"] > thr).sum()) >= 1 and int((g["rewards"] < thr).sum()) >= 1
    assert int(((g["rewards"] > 0) & (g["rewards"] < thr)).sum()) >= 1, "no reward strictly between 0 and the threshold"


@pytest.mark.parametrize("tag", CASES)
def test_stored_reward_state_follows_the_stored_rewards(F, tag):
    g = case(F, tag)
    rs = np.zeros(g["rewards"].shape[1], np.uint8)
    for t in range(g["rewards"].shape[0]):
        rs = np.minimum(rs + (g["rewards"][t] - float(g["threshold"]) > 0) * 255, 255)  # ants.py:119-121
        np.testing.assert_array_equal(g["reward_state_step"][t], rs, err_msg="%s step %d" % (tag, t))
        rs = (rs * 0.9).astype(np.uint8)                                                 # ants.py:130
        np.testing.assert_array_equal(g["reward_state_update"][t], rs, err_msg="%s update %d" % (tag, t))


@pytest.mark.parametrize("tag", CASES)
def test_the_probe_replayed_on_the_stored_coordinates_returns_the_stored_rewards(F, tag):
    g = case(F, tag)
    c = g["obs_coords"].astype(np.int64)
    P = c.shape[2]
    unmasked = np.broadcast_to(g["mask"].astype(bool) if tag == "mask" else np.ones((P, P), bool), c.shape[1:4])
    food = np.unpackbits(g["food_seen"], axis=-1)[..., :P].astype(bool)
    visits = np.zeros((1, W, H), np.int64)
    r0 = probe_reward(visits, c[0], unmasked, food[0], g["holding_seen"][0])
    np.testing.assert_array_equal(r0, g["reward_observation0"], err_msg="%s: the initial observation" % tag)
    for t in range(g["rewards"].shape[0]):
        r = probe_reward(visits, c[t + 1], unmasked, food[t + 1], g["holding_seen"][t + 1]) - 0.25 * (g["rot"][t] != 0)
        np.testing.assert_array_equal(r, g["rewards"][t], err_msg="%s: step %d" % (tag, t))
    assert (visits > 0).sum() > c.shape[1] * 4  # (the visits map filled as the ants moved)
