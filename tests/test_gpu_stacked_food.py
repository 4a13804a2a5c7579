"""k_update_move on food cells shared by ants of different waves (tests/stacked_food.py).

Each case is driven once, the way bench.py drives the device — reset, then step_update(rot, ph, None) every step with no
read in between, so from step 2 on every update rides inside the next step's k_update_move — and then held to the oracle:
reward, done and agent_state exactly and the observation through check_obs after every step, the complete state after the
last one.  tests/test_stacked_food_cpu.py certifies, on these very runs, that each contains at least 20 pickups that empty a
cell shared across waves and at least 20 drops on shared anthill cells in its deferred steps, and that one ant reading its
cell after the winner's write would change holding and mandibles, which are compared exactly here.

Four cases run k_update_move<2, false> (explicit sweep or a filter with a radius: 8-byte {food, META} records beside separate
pheromone buffers; 4 x 4-tiled on 32 x 32, row-major on 30 x 34 and 28 x 36; 16 waves, a last wave of two ants, rocks), the
fifth k_update_move<2, true> (scaled units, interleaved records) as the control.  Nothing here is repeated to chase a timing:
the run is deterministic wherever the kernel orders its food reads ahead of its food writes."""
import numpy as np
import pytest

import stacked_food as sf
from helpers import assert_xy_close, phero_close
from test_gpu_parity import XY_ATOL, _cpu, check_obs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(sf.CASES))
def test_contended_food_cells_follow_the_oracle(case):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    cfg = sf.case_cfg(case)
    init = sf.stacked_init(cfg, sf.case_seed(case))
    rot, ph = sf.stacked_actions(cfg, sf.STEPS, sf.case_seed(case) + 1)
    E = cfg.n_envs
    env = BatchedAntsEnv(cfg)
    assert env.query(cm.Q_CELL_META) == 1 and env.query(cm.Q_DEFERRED_UPDATE) == 1
    # which instantiation of k_update_move the case is there for (antsrl_launch_update_move: interleaved records or not)
    scaled = sf.CASES[case][4] == "scaled"
    assert env.query(cm.Q_INTERLEAVED) == int(scaled) and env.query(cm.Q_SCALED_UNITS) == int(scaled)
    env.reset(init)
    # the device first (nothing but step_update touches the handle), its outputs kept on the device; then the oracle
    got = [[x.clone() for x in env.step_update(rot[t], ph[t], None)] for t in range(sf.STEPS)]
    r = sf.oracle_run(case, n_threads=E)
    np.testing.assert_array_equal(r["rot"], rot)
    want, orc = r["outs"], r["oracle"]
    assert len(got) == len(want) == sf.STEPS
    for s, ((obs, ast, rew, done), (o_obs, o_ast, o_rew, o_done)) in enumerate(zip(got, want)):
        ctx = "%s step %d" % (case, s)
        np.testing.assert_array_equal(_cpu(rew), o_rew.astype(np.float32), err_msg=ctx + " reward")
        np.testing.assert_array_equal(_cpu(done), o_done, err_msg=ctx + " done")
        np.testing.assert_array_equal(_cpu(ast), o_ast.astype(np.float32), err_msg=ctx + " agent_state")
        go = _cpu(obs)
        for e in range(E):
            check_obs(cfg, go[e], o_obs[e], ctx + " env %d" % e)
    # the complete state after the last step (this read enqueues the last deferred update)
    ctx = case + " final"
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_HOLDING)), orc.holding, err_msg=ctx + " holding")
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_MANDIBLES)), orc.mandibles, err_msg=ctx + " mandibles")
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_FOOD)), orc.food, err_msg=ctx + " food")
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_ANTHILL_FOOD)), orc.anthill_food, err_msg=ctx + " anthill_food")
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_EXPLORED)), orc.explored, err_msg=ctx + " explored")
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_TIMESTEP)), orc.timestep, err_msg=ctx + " timestep")
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_REWARD_STATE)), orc.reward_state, err_msg=ctx + " reward_state")
    xyt = _cpu(env.read_state(cm.S_ANTS_XYT))
    assert_xy_close(xyt, orc.ants_xyt, XY_ATOL, ctx)
    np.testing.assert_array_equal(np.floor(xyt[..., :2]), np.floor(orc.ants_xyt[..., :2]), err_msg=ctx + " cells")
    assert_xy_close(_cpu(env.read_state(cm.S_PREV_XY)), np.stack([orc.prev_x, orc.prev_y], -1), XY_ATOL, ctx + " prev")
    ok = phero_close(_cpu(env.read_state(cm.S_PHERO)), orc.phero, threshold=cfg.phero_threshold)
    assert ok.all(), "%s pheromone: %d cells off" % (ctx, (~ok).sum())
    if cfg.n_rocks:
        assert_xy_close(_cpu(env.read_state(cm.S_ROCK_CENTERS)), orc.rock_centers, XY_ATOL, ctx + " rocks")
