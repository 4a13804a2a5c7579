"""The deferred update (k_update_move) on the crowd fixtures' states.

test_hip_matches_reference_golden reads the state after every op and injects the recorded jitter, so every update of a
recording runs in k_update_one.  Here the device is driven the way bench.py drives it — step_update(rot, ph, None) every
step and no state read in between, so every update rides inside the next step's k_update_move — from the initial state and
with the actions of each crowd recording (ants on the borders, on wall cells, under overlapping rocks, 64 to 192 cells).
Three environments with a non-zero env_id_base draw different wall jitter and diverge; the oracle draws the same jitter
from the same generator.  tests/test_crowd_fixtures_cpu.py certifies what these very runs contain.
Every recording runs twice: as recorded (scaled units and interleaved records everywhere but c03, whose filter has a radius:
k_update_move<2, true>) and with AntsCfg.phero_mode = PHERO_EXPLICIT_SWEEP ({food, META} records beside separate pheromone
buffers: k_update_move<2, false>) — the reference's semantics do not depend on the mode, so the oracle's run is the same.

The variant recordings (tests/golden/v*.npz: carry, backward, speed, rotation, threshold and weights off their defaults,
other masks) are driven the same way wherever the handle defers the update (Q_DEFERRED_UPDATE): k_update_move carries its
own copy of the move (`fwd < 0 -> fwd * backward`), which nothing else reaches.  A shape the cell-meta path refuses would take
ACT_AUTO, which never defers: those recordings (v06-v11) are no cases here, the golden replay runs them; a rotation-only
recording would pass no pheromone actions.  tests/test_variant_fixtures_cpu.py certifies that the
oracle's runs here contain the backward move and rewards between each threshold and 1."""
import numpy as np
import pytest

import crowd_events as ce
from helpers import assert_xy_close, crowd_fixture_names, load_fixture, phero_close, variant_fixture_names
from test_crowd_fixtures_cpu import ENV_ID_BASE, N_ENVS
from test_variant_fixtures_cpu import is_backward_file
from test_gpu_parity import XY_ATOL, _cpu, check_obs

pytestmark = pytest.mark.gpu


def test_both_perceive_paths_are_among_the_cases():
    shapes = [(m["w"], m["h"]) for m in (load_fixture(n)[3] for n in crowd_fixture_names())]
    assert (64, 64) in shapes and any(w & (w - 1) or h & (h - 1) for w, h in shapes)


def _variant_handle(cfg):
    """A variant recording's handle: the cell-meta path where it takes the shape, else the library's own choice."""
    from antsrl_amd import _lib, config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    cfg.act_path = cm.ACT_CELL_META
    try:
        return BatchedAntsEnv(cfg)
    except _lib.AntsrlError as e:
        if "ANTSRL_ACT_CELL_META" not in str(e):
            raise
    cfg.act_path = cm.ACT_AUTO
    return BatchedAntsEnv(cfg)


def _defers(meta, mask):
    """The library's conditions for k_update_move (antsrl_update_move_supported: the cell-meta layout, two pheromones, at
    most 1024 ants), restated on a recording's meta so that the cases below can be chosen at collection: the generator's
    channel order, 128..368 observation values per ant over at most 64 cells.  The test right below holds it to the library."""
    order = ["Ants", "Pheromone", "Pheromone", "Anthill", "Walls", "Food"] + (["CircleObstacles"] if meta["n_rocks"] else [])
    cells = (2 * meta.get("radius", mask.shape[0] // 2) + 1) ** 2
    return (meta["n_phero"] == 2 and meta["perceived"] == order and meta.get("perceived_arg", [0, 0, 1])[1:3] == [0, 1]
            and cells <= 64 and 128 <= cells * len(order) <= 368 and meta["n_ants"] <= 1024)


def deferring_variant_names():
    out = []
    for name in variant_fixture_names():
        cfg, init, F, meta = load_fixture(name)
        if _defers(meta, F["mask"]):
            out.append(name)
    return out


def test_the_backward_move_and_the_threshold_run_deferred():
    """The variant recordings driven below are exactly those whose handle defers the update (a shape the cell-meta path
    refuses takes ACT_AUTO, which never defers); at least one backward-motion recording and the threshold / weights
    recording are among them."""
    from antsrl_amd import config as cm
    deferred = []
    for name in variant_fixture_names():
        cfg, init, F, meta = load_fixture(name, N_ENVS)
        if _variant_handle(cfg).query(cm.Q_DEFERRED_UPDATE) == 1:
            deferred.append(meta)
    assert [m["name"] for m in deferred] == deferring_variant_names()
    assert any(is_backward_file(m) for m in deferred)
    assert any(m["reward_threshold"] < 1 and m["max_speed"] == 2.5 and m["reward"] == "all" for m in deferred)


def _cases():
    """(name, phero_mode): every recording as recorded, under its name as the case's id, and once more under the explicit sweep."""
    names = crowd_fixture_names() + deferring_variant_names()
    return ([pytest.param(n, "as_recorded", id=n) for n in names] +
            [pytest.param(n, "explicit_sweep", id=n + "-explicit_sweep") for n in names])


@pytest.mark.parametrize("name,phero_mode", _cases())
def test_deferred_path_follows_the_oracle_on_crowd_states(name, phero_mode):
    """explicit_sweep: the same recording with AntsCfg.phero_mode = PHERO_EXPLICIT_SWEEP — the reference's semantics do not
    depend on it, so the oracle's run is the same; the device keeps 8-byte {food, META} records beside separate pheromone
    buffers and every deferred update runs in k_update_move<2, false> (as recorded only c03's filter has a radius)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    cfg, init, F, meta = load_fixture(name, N_ENVS)
    cfg.env_id_base = ENV_ID_BASE
    explicit = phero_mode == "explicit_sweep"
    if explicit:
        cfg.phero_mode = cm.PHERO_EXPLICIT_SWEEP
    E, N = N_ENVS, cfg.n_ants
    if name in variant_fixture_names():
        env = _variant_handle(cfg)
        assert env.query(cm.Q_CELL_META) == 1 and env.query(cm.Q_DEFERRED_UPDATE) == 1
    else:
        cfg.act_path = cm.ACT_CELL_META
        env = BatchedAntsEnv(cfg)
        assert env.query(cm.Q_CELL_META) == 1 and env.query(cm.Q_DEFERRED_UPDATE) == 1
        pow2 = not (cfg.w & (cfg.w - 1) or cfg.h & (cfg.h - 1))
        if explicit:  # (include/antsrl.h, ANTSRL_Q_PERCEIVE_FAST: the fast path reads interleaved records, which a sweep does not keep)
            assert env.query(cm.Q_PERCEIVE_FAST) == 0, "generic k_perceive on the explicit-sweep layout"
        else:
            assert env.query(cm.Q_PERCEIVE_FAST) == int(pow2), "fast k_perceive on power-of-two grids with the default mask, else generic"
    if explicit:
        assert env.query(cm.Q_SCALED_UNITS) == 0 and env.query(cm.Q_INTERLEAVED) == 0
    env.reset(init)
    if meta["deposit_strength"] != 1.0:
        env.set_activation(np.broadcast_to(F["init_activation"], (E,) + F["init_activation"].shape).copy(),
                           meta["deposit_strength"])
    # the device first (nothing but step_update touches the handle), its outputs kept on the device; then the oracle
    got = []
    for t in np.nonzero(F["ops"] == ce.OP_STEP)[0]:
        rot = np.broadcast_to(F["rot"][t], (E, N))
        ph = np.broadcast_to(F["ph"][t], (E, N)) if F["has_ph"][t] else None
        got.append([x.clone() for x in env.step_update(rot, ph, None)])
    trs, want, orc = ce.oracle_deferred_run(cfg, init, F, meta, ENV_ID_BASE, n_threads=N_ENVS)
    assert len(got) == len(want)
    for s, ((obs, ast, rew, done), (o_obs, o_ast, o_rew, o_done)) in enumerate(zip(got, want)):
        ctx = "%s step %d" % (name, s)
        np.testing.assert_array_equal(_cpu(rew), o_rew.astype(np.float32), err_msg=ctx + " reward")
        np.testing.assert_array_equal(_cpu(done), o_done, err_msg=ctx + " done")
        np.testing.assert_array_equal(_cpu(ast), o_ast.astype(np.float32), err_msg=ctx + " agent_state")
        go = _cpu(obs)
        for e in range(E):
            check_obs(cfg, go[e], o_obs[e], ctx + " env %d" % e)
    # the complete state after the last step (this read enqueues the last deferred update)
    ctx = name + " final"
    xyt = _cpu(env.read_state(cm.S_ANTS_XYT))
    assert_xy_close(xyt, orc.ants_xyt, XY_ATOL, ctx)
    np.testing.assert_array_equal(np.floor(xyt[..., :2]), np.floor(orc.ants_xyt[..., :2]), err_msg=ctx + " cells")
    assert_xy_close(_cpu(env.read_state(cm.S_PREV_XY)), np.stack([orc.prev_x, orc.prev_y], -1), XY_ATOL, ctx + " prev")
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_HOLDING)), orc.holding, err_msg=ctx)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_MANDIBLES)), orc.mandibles, err_msg=ctx)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_FOOD)), orc.food, err_msg=ctx)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_EXPLORED)), orc.explored, err_msg=ctx)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_ANTHILL_FOOD)), orc.anthill_food, err_msg=ctx)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_TIMESTEP)), orc.timestep, err_msg=ctx)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_REWARD_STATE)), orc.reward_state, err_msg=ctx)
    ok = phero_close(_cpu(env.read_state(cm.S_PHERO)), orc.phero, threshold=cfg.phero_threshold)
    assert ok.all(), "%s pheromone: %d cells off" % (ctx, (~ok).sum())
    if cfg.n_rocks:
        assert_xy_close(_cpu(env.read_state(cm.S_ROCK_CENTERS)), orc.rock_centers, XY_ATOL, ctx + " rocks")
