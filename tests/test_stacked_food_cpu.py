"""Certifies on the CPU oracle what tests/test_gpu_stacked_food.py runs on the device (tests/stacked_food.py): every case,
driven exactly as the device is driven, contains exchanges on food cells shared by ants of different waves — pickups that
empty the cell and drops on the anthill area — in the steps whose move runs inside k_update_move; one ant reading such a
cell after the winner's write would change what the GPU test compares exactly; and no coordinate sits where a last-ulp
difference flips a cell."""
import numpy as np
import pytest

import stacked_food as sf
from test_crowd_fixtures_cpu import MIN_DISTANCE_TO_INTEGER

#: contended pickups / drops every case must contain in its deferred steps
FLOOR = 20


@pytest.fixture(scope="module")
def runs():
    return {case: sf.oracle_run(case) for case in sf.CASES}


def _sensitive(cfg, cell):
    k = sf.late_reader(cell)
    return k is not None and sf.late_read_changes_the_outcome(cell["food"], cell["on_area"], cell["mandibles"],
                                                              cell["holding"], cfg.max_hold, k)


def test_the_cases_cover_both_record_layouts_and_a_ragged_wave():
    shapes = [sf.CASES[c][:3] for c in sf.CASES]
    assert any(w % 4 or h % 4 for _, w, h in shapes), "row-major {food, META} records (KP::ftile == 0)"
    assert any(w % 4 == 0 and h % 4 == 0 for _, w, h in shapes), "4 x 4-tiled records (KP::ftile == 1)"
    assert any(n == 1024 for n, _, _ in shapes), "16 waves"
    assert any(n == 130 for n, _, _ in shapes), "a last wave of two ants"
    assert any(sf.CASES[c][3] for c in sf.CASES) and any(sf.CASES[c][4] == "scaled" for c in sf.CASES)
    assert sum(sf.CASES[c][4] != "scaled" for c in sf.CASES) >= 3


@pytest.mark.parametrize("case", list(sf.CASES))
def test_contended_exchanges_reach_their_floors_in_the_deferred_steps(runs, case):
    """Counted from stacked_food.FIRST_DEFERRED_STEP on: the handle's first update after a reset is never deferred, so the
    first k_update_move is step 2's."""
    r = runs[case]
    per_step = [(len(p), len(d)) for p, d in r["contended"]]
    pickups = sum(p for p, _ in per_step[sf.FIRST_DEFERRED_STEP:])
    drops = sum(d for _, d in per_step[sf.FIRST_DEFERRED_STEP:])
    print("%s: contended pickups %d, contended drops %d in steps %d..%d; per step %s"
          % (case, pickups, drops, sf.FIRST_DEFERRED_STEP, sf.STEPS - 1, per_step))
    assert pickups >= FLOOR and drops >= FLOOR


@pytest.mark.parametrize("case", list(sf.CASES))
def test_one_late_read_would_change_what_the_gpu_test_compares(runs, case):
    """At least one deferred step in which EVERY counted cell, pickups and drops alike, is sensitive to one late read; and,
    over all deferred steps, sensitive pickup cells and sensitive drop cells each reach the floor by themselves."""
    r = runs[case]
    whole_steps, n_pick, n_drop = [], 0, 0
    for t in range(sf.FIRST_DEFERRED_STEP, sf.STEPS):
        p, d = r["contended"][t]
        sp, sd = [_sensitive(r["cfg"], c) for c in p], [_sensitive(r["cfg"], c) for c in d]
        n_pick += sum(sp)
        n_drop += sum(sd)
        if p and d and all(sp) and all(sd):
            whole_steps.append(t)
    print("%s: late-read-sensitive pickup cells %d, drop cells %d; steps with every counted cell sensitive: %s"
          % (case, n_pick, n_drop, whole_steps))
    assert whole_steps
    assert n_pick >= FLOOR and n_drop >= FLOOR


def test_the_restated_exchange():
    """late_read_changes_the_outcome on cells worked out by hand."""
    # two open ants on 3 units: both take 3, the cell is left empty; the late one would see 0 and take nothing
    assert sf.late_read_changes_the_outcome(3.0, False, [0, 0], [0.0, 0.0], 5.0, 0)
    # 7 units: the winner leaves 2, the late one still closes (and takes 2, not 5)
    assert sf.late_read_changes_the_outcome(7.0, False, [0, 0], [0.0, 0.0], 5.0, 0)
    # two carriers on the area: both drop; the late one would see the winner's food and stay closed
    assert sf.late_read_changes_the_outcome(0.0, True, [1, 1], [3.0, 3.0], 5.0, 0)
    # the winner is a carrier off the area: it writes nothing, a late read sees what everyone saw
    assert not sf.late_read_changes_the_outcome(3.0, False, [0, 0, 1], [0.0, 0.0, 2.0], 5.0, 0)
    # a late reader that is already closed off the area stays closed whatever it reads
    assert not sf.late_read_changes_the_outcome(3.0, False, [1, 0, 0], [2.0, 0.0, 0.0], 5.0, 0)


@pytest.mark.parametrize("case", list(sf.CASES))
def test_the_groups_are_stacked_across_every_wave_at_the_start(case):
    cfg = sf.case_cfg(case)
    init = sf.stacked_init(cfg, sf.case_seed(case))
    N, G = cfg.n_ants, min(sf.WAVE, cfg.n_ants)
    xyt, area = init["ants_xyt"], sf.anthill_area(cfg, init)
    np.testing.assert_array_equal(xyt, xyt[:, np.arange(N) % G])
    frac = xyt[..., :2] - np.floor(xyt[..., :2])
    assert frac.min() >= 0.2 - 1e-12 and frac.max() <= 0.8 + 1e-12
    cx, cy = xyt[..., 0].astype(int), xyt[..., 1].astype(int)
    e = np.arange(cfg.n_envs)[:, None]
    assert not init["walls"][e, cx, cy].any() and not (init["walls"].astype(bool) & area).any()
    on = area[e, cx, cy][:, :G].mean()
    assert 0.4 <= on <= 0.6, "about half the groups start on the anthill area"
    assert (init["food"][area] == 0).all() and (init["food"][~area & ~init["walls"].astype(bool)] > 0).all()
    rot, ph = sf.stacked_actions(cfg, sf.STEPS, sf.case_seed(case) + 1)
    np.testing.assert_array_equal(rot, rot[:, :, np.arange(N) % G])
    assert (ph != ph[:, :, np.arange(N) % G]).any(), "pheromone actions are drawn per ant"


@pytest.mark.parametrize("case", list(sf.CASES))
def test_no_coordinate_next_to_an_integer(runs, case):
    xy = runs[case]["xy"]
    d = float(np.abs(xy - np.round(xy)).min())
    print(case, d)
    assert d >= MIN_DISTANCE_TO_INTEGER
