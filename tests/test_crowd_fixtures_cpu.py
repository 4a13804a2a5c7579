"""Certifies, from their arrays alone, that the crowd fixtures (tests/golden/c*.npz and oracle_only/) contain what they
were recorded for, and that the GPU can be held to them: every event class of crowd_events.FLOORS reaches its floor in
at least one recording AND in at least one oracle run driven the way tests/test_gpu_crowd_deferred.py drives the device;
no file is large; no coordinate sits where a last-ulp difference flips a cell; a one-ulp change of the initial state stays
a hundred times below the GPU's coordinate tolerance."""
import os

import numpy as np
import pytest

import crowd_events as ce
from helpers import GOLDEN, crowd_fixture_names, load_fixture, oracle_only_fixture_names

#: the deferred-path runs (here on the oracle, in test_gpu_crowd_deferred.py on the device): three environments that
#: draw the library's wall jitter as global environments 5, 6 and 7
N_ENVS, ENV_ID_BASE = 3, 5
MAX_BYTES = 2_000_000
MIN_DISTANCE_TO_INTEGER = 1e-6
SENSITIVITY_BOUND = 1e-11  # 1 % of test_gpu_parity.XY_ATOL

NEW = crowd_fixture_names() + oracle_only_fixture_names()


@pytest.fixture(scope="module")
def recorded():
    """name -> (trajectory, event counts) of every new recording."""
    out = {}
    for name in NEW:
        cfg, init, F, meta = load_fixture(name)
        tr = ce.from_fixture(F, meta, init)
        out[name] = (tr, ce.count_events(tr))
    return out


@pytest.fixture(scope="module")
def deferred_runs():
    """name -> (per-env trajectories, per-env trajectories from the nudged start) of every GPU-replayed new recording."""
    out = {}
    for name in crowd_fixture_names():
        cfg, init, F, meta = load_fixture(name, N_ENVS)
        out[name] = (ce.oracle_deferred_run(cfg, init, F, meta, ENV_ID_BASE)[0],
                     ce.oracle_deferred_run(cfg, init, F, meta, ENV_ID_BASE, nudge=True)[0])
    return out


def test_the_issue_s_scenarios_are_there():
    metas = {n: load_fixture(n)[3] for n in NEW}
    gpu = {n: m for n, m in metas.items() if not n.startswith("oracle_only/")}
    assert 5 <= len(gpu) <= 6 and len(metas) == len(gpu) + 1
    steps = {n: int((load_fixture(n)[2]["ops"] == ce.OP_STEP).sum()) for n in NEW}
    assert any(m["n_rocks"] and m["placed_ants"] and m["placed_rocks"] for m in gpu.values())
    assert any(m["wall_density"] >= 0.3 and m["n_rocks"] and m["deposit_strength"] != 1.0 and m["reward"] == "all"
               for m in gpu.values())
    assert any(m["n_rocks"] and np.count_nonzero(m["filter"]) == 9 for m in gpu.values())
    assert any(max(m["w"], m["h"]) <= 16 and m["n_ants"] >= 64 and m["h"] % 8 for m in gpu.values())
    assert any(m["rich_food"] and m["n_rocks"] and m["max_hold"] == 5 for m in gpu.values())
    assert any(m["n_rocks"] == 0 and steps[n] >= 600 for n, m in gpu.items())
    assert all(steps[n] <= 120 or m["n_rocks"] == 0 for n, m in gpu.items()), "what the GPU replays: <= 120 steps or no rocks"
    assert any(m["n_rocks"] and steps[n] >= 400 for n, m in metas.items() if n.startswith("oracle_only/"))


@pytest.mark.parametrize("event", sorted(ce.FLOORS))
def test_event_floor_in_a_recording(recorded, event):
    counts = {name: c[event] for name, (_, c) in recorded.items()}
    print(event, counts)
    assert max(counts.values()) >= ce.FLOORS[event], counts


@pytest.mark.parametrize("event", sorted(ce.FLOORS))
def test_event_floor_in_a_deferred_run(deferred_runs, event):
    counts = {name: [ce.count_events(tr)[event] for tr in trs] for name, (trs, _) in deferred_runs.items()}
    print(event, counts)
    assert max(max(v) for v in counts.values()) >= ce.FLOORS[event], counts


def test_the_deferred_runs_diverge(deferred_runs):
    for name, (trs, _) in deferred_runs.items():
        assert not np.array_equal(trs[0]["ants"][-1], trs[1]["ants"][-1]), name
        assert not np.array_equal(trs[1]["ants"][-1], trs[2]["ants"][-1]), name


@pytest.mark.parametrize("name", NEW)
def test_size(name):
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= MAX_BYTES


@pytest.mark.parametrize("name", NEW)
def test_no_coordinate_next_to_an_integer(recorded, name):
    d = ce.min_distance_to_integer(recorded[name][0])
    print(name, d)
    assert d >= MIN_DISTANCE_TO_INTEGER


@pytest.mark.parametrize("name", crowd_fixture_names())
def test_no_coordinate_next_to_an_integer_in_the_deferred_runs(deferred_runs, name):
    d = min(ce.min_distance_to_integer(tr) for tr in deferred_runs[name][0])
    print(name, d)
    assert d >= MIN_DISTANCE_TO_INTEGER


def _largest_difference(a, b):
    return max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()) if a[1].size else 0.0)


@pytest.mark.parametrize("name", crowd_fixture_names())
def test_one_ulp_sensitivity_of_the_replay(name):
    """The oracle replays the recording twice, the second time with every ant's x and theta one ulp up: ant coordinates,
    headings and rock centres after every op stay within SENSITIVITY_BOUND."""
    cfg, init, F, meta = load_fixture(name)
    first = ce.oracle_replay_coordinates(cfg, init, F, meta)
    np.testing.assert_array_equal(first[0], F["ants"])
    d = _largest_difference(first, ce.oracle_replay_coordinates(cfg, init, F, meta, nudge=True))
    print(name, d)
    assert d <= SENSITIVITY_BOUND


@pytest.mark.parametrize("name", crowd_fixture_names())
def test_one_ulp_sensitivity_of_the_deferred_runs(deferred_runs, name):
    d = max(_largest_difference((a["ants"], a["rock_centers"]), (b["ants"], b["rock_centers"]))
            for a, b in zip(*deferred_runs[name]))
    print(name, d)
    assert d <= SENSITIVITY_BOUND
