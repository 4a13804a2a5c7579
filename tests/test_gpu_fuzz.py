"""Randomised configurations against the oracle: perception radius 1..7 (one and several passes), random
masks, channel lists in any order with repeats (generic layout), 1..4 pheromone channels, 0..4 rocks,
every reward kind, diffusion filters of radius 0..2 in both pheromone modes, ragged grids and ant
counts, forward shifts.  Each case is a few steps of step + update with injected wall-jitter draws.

Everything here is held to the ORACLE.  The oracle's own reading of these parameters is pinned to the reference by the
recordings under tests/golden/ at the values listed in tests/test_gpu_parity.py's docstring (one or two per parameter:
masks of side 5, 7 and 11, no mask at radius 5, DELTA 1.37, reordered and repeated channels, max_hold 2, max_val 100 / None,
1 and 3 pheromones, carry, backward, speed, rotation, threshold and weights off their defaults); the other values drawn
here (radius 1, 4, 6, 7, four pheromones, backward 0 / 1, threshold 0 / 2.5, no rotation) rest on the oracle alone.
test_random_motion_and_reward_parameters_vs_oracle is the one test that moves carry, backward, rotation speed, threshold
and All_Rewards' weights."""
import numpy as np
import pytest

from test_gpu_parity import _anthill_dist, _check_reward, _compare_with_oracle, _cpu, check_obs, torch_mod  # noqa: F401  (the parity suite's checks and fixture)

pytestmark = pytest.mark.gpu


def _random_case(rng):
    from antsrl_amd import config as cm
    E = int(rng.integers(1, 4))
    N = int(rng.choice([1, 7, 64, 65, 130, 257, 600, 1025, 1100]))
    W, H = int(rng.integers(12, 90)), int(rng.integers(12, 90))
    r = int(rng.integers(1, 8))
    n_phero = int(rng.choice([2, 2, 2, 1, 3, 4]))
    n_rocks = int(rng.integers(0, 5))
    kinds_pool = [cm.CH_ANTS, cm.CH_ANTHILL, cm.CH_WALLS, cm.CH_FOOD] + [cm.CH_PHERO] * 2 + ([cm.CH_ROCKS] if n_rocks else [])
    K = int(rng.integers(1, 10))
    channels = []
    for _ in range(K):
        k = int(rng.choice(kinds_pool))
        channels.append((k, int(rng.integers(0, n_phero)) if k == cm.CH_PHERO else 0))
    if rng.random() < 0.35:
        channels = None  # the generator's default layout
    mask = None if rng.random() < 0.3 else (rng.random((2 * r + 1, 2 * r + 1)) < 0.8)
    fr = int(rng.choice([0, 0, 1, 2]))
    if fr == 0:
        filt = np.array([[float(rng.choice([0.999, 0.9, 1.0]))]])
    else:
        filt = rng.random((2 * fr + 1, 2 * fr + 1))
        if rng.random() < 0.4:  # rank-1: the separable form of the stencil
            filt = np.outer(rng.random(2 * fr + 1), rng.random(2 * fr + 1))
        filt = filt / filt.sum() * float(rng.choice([0.999, 0.95]))
    kw = dict(n_phero=n_phero, n_rocks=n_rocks, mask=mask, perception_radius=r, channels=channels,
              fwd_delta=float(rng.choice([0.0, 4.0, 2.5])), deposit_strength=float(rng.choice([1.0, 256.0])),
              filt=filt, reward_kind=int(rng.integers(0, 4)), fct_explore_holding=float(rng.choice([0.0, 0.5])),
              phero_mode=int(rng.integers(0, 2)), max_time=int(rng.choice([3, 2000])),
              delta=float(rng.choice([1.1, 1.1, 1.0, 1.37])), max_speed=float(rng.choice([1.0, 2.5])),
              max_hold=float(rng.choice([5.0, 2.0])))
    if channels is not None and not any(k == cm.CH_PHERO for k, _ in channels) and rng.random() < 0.5:
        kw["phero_max_val"] = None  # Pheromone(max_val=None): legal as long as no pheromone is perceived
    return E, N, W, H, kw


# a longer one-off campaign:  ANTSRL_FUZZ_BASE=64 ANTSRL_FUZZ_CASES=2000 python -m pytest tests/test_gpu_fuzz.py -m gpu -q
import os
_BASE, _CASES = int(os.environ.get("ANTSRL_FUZZ_BASE", "0")), int(os.environ.get("ANTSRL_FUZZ_CASES", "64"))


@pytest.mark.parametrize("seed", range(_BASE, _BASE + _CASES))
def test_random_configuration_vs_oracle(torch_mod, seed):
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    from oracle.oracle import Oracle
    rng = np.random.default_rng(1000 + seed)
    E, N, W, H, kw = _random_case(rng)
    cfg = cm.make_cfg(E, N, W, H, **kw)
    init = synth_init(cfg, seed=seed, n_food_discs=4, food_rmin=1, food_rmax=4, wall_density=0.08)
    if cfg.n_phero == 2:
        _compare_with_oracle(torch_mod, cfg, init, steps=5, seed=seed, jitter_mode="injected")
        return
    # pheromone actions need exactly two channels (ants.py:89-96): rotation only, activation set directly
    env, orc = BatchedAntsEnv(cfg), Oracle(cfg, init)
    env.reset(init)
    act = rng.choice([0.0, 10.0], size=(E, N, cfg.n_phero)).astype(np.float32)
    env.set_activation(act)
    orc.set_activation(act)
    prev_dist = _anthill_dist(init, orc.ants_xyt)
    for t in range(5):
        rot = rng.integers(-1, 2, (E, N), dtype=np.int8)
        jit = rng.random((E, N))
        obs, ast, rew, done = env.step(rot, None)
        o_obs, o_ast, o_rew, o_done = orc.step(rot, None)
        for e in range(E):
            check_obs(cfg, _cpu(obs)[e], o_obs[e], "seed %d step %d env %d" % (seed, t, e))
        _check_reward(cfg, init, _cpu(rew), o_rew, orc.ants_xyt, prev_dist, "seed %d step %d" % (seed, t))
        prev_dist = _anthill_dist(init, orc.ants_xyt)
        np.testing.assert_array_equal(_cpu(done), o_done)
        env.update(jit)
        orc.update(jit)
    from helpers import phero_close
    assert phero_close(_cpu(env.read_state(cm.S_PHERO)), orc.phero, threshold=cfg.phero_threshold).all()
    np.testing.assert_allclose(_cpu(env.read_state(cm.S_ANTS_XYT)), orc.ants_xyt, rtol=0, atol=1e-9)


@pytest.mark.parametrize("seed", range(100, 124))
def test_random_configuration_fused_calls_and_standalone_observation(torch_mod, seed):
    """The same random configurations driven the way main.py does: antsrl_step_update (one call per
    step), a standalone observation before the first step and after some updates (main.py:88), and a
    step without pheromone actions."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    from oracle.oracle import Oracle
    rng = np.random.default_rng(1000 + seed)
    E, N, W, H, kw = _random_case(rng)
    kw["n_phero"] = 2
    if kw["channels"] is not None:
        kw["channels"] = [(k, a % 2) for k, a in kw["channels"]]
    cfg = cm.make_cfg(E, N, W, H, **kw)
    init = synth_init(cfg, seed=seed, n_food_discs=4, food_rmin=1, food_rmax=4, wall_density=0.08)
    env, orc = BatchedAntsEnv(cfg), Oracle(cfg, init)
    env.reset(init)

    def same_obs(got, want, ctx):
        g = _cpu(got)
        for e in range(E):
            check_obs(cfg, g[e], want[e], "seed %d %s env %d" % (seed, ctx, e))

    prev_dist = [_anthill_dist(init, orc.ants_xyt)]

    def same_reward(got, want, ctx):  # (bit-exact but for heading-term ties, see _check_reward)
        _check_reward(cfg, init, _cpu(got), want, orc.ants_xyt, prev_dist[0], "seed %d %s" % (seed, ctx))
        prev_dist[0] = _anthill_dist(init, orc.ants_xyt)

    obs, ast, rew = env.observe()
    o_obs, o_ast, o_rew = orc.observe()
    same_obs(obs, o_obs, "first observation")
    same_reward(rew, o_rew, "first observation")
    for t in range(6):
        rot = rng.integers(-1, 2, (E, N), dtype=np.int8)
        ph = rng.integers(0, 3, (E, N), dtype=np.int8) if t != 3 else None
        jit = rng.random((E, N))
        obs, ast, rew, done = env.step_update(rot, ph, jit)
        o_obs, o_ast, o_rew, o_done = orc.step(rot, ph)
        same_obs(obs, o_obs, "step %d" % t)
        np.testing.assert_array_equal(_cpu(ast), o_ast.astype(np.float32))
        same_reward(rew, o_rew, "step %d" % t)
        np.testing.assert_array_equal(_cpu(done), o_done)
        orc.update(jit)
        if t in (1, 4):
            obs, ast, rew = env.observe()
            o_obs, o_ast, o_rew = orc.observe()
            same_obs(obs, o_obs, "observation after update %d" % t)
            same_reward(rew, o_rew, "observation after update %d" % t)
    from helpers import phero_close
    assert phero_close(_cpu(env.read_state(cm.S_PHERO)), orc.phero, threshold=cfg.phero_threshold).all()
    np.testing.assert_allclose(_cpu(env.read_state(cm.S_ANTS_XYT)), orc.ants_xyt, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_FOOD)), orc.food)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_ANTHILL_FOOD)), orc.anthill_food)


@pytest.mark.parametrize("seed", range(200, 208))
def test_random_configuration_on_grids_past_the_lds_limit(torch_mod, seed):
    """The random configurations on grids of 0.7–1.2 M cells: presence / explored maps in HBM scratch
    (k_act<..., BIG>), every reward kind, masks, channel lists, rocks, both pheromone modes at radius 0."""
    from antsrl_amd import config as cm
    from antsrl_amd.synth import synth_init
    rng = np.random.default_rng(3000 + seed)
    E, N, W, H, kw = _random_case(rng)
    E, N = 1, int(rng.choice([1, 40, 130, 600]))
    W, H = int(rng.integers(700, 1100)), int(rng.integers(900, 1100))
    kw["n_phero"] = 2
    if kw["channels"] is not None:
        kw["channels"] = [(k, a % 2) for k, a in kw["channels"]]
    if np.asarray(kw["filt"]).shape[0] > 1:
        kw["filt"] = np.array([[0.999]])  # keep the oracle's stencil over a million cells out of the test's time
    kw["perception_radius"] = min(kw["perception_radius"], 5)
    if kw["mask"] is not None:
        p = 2 * kw["perception_radius"] + 1
        kw["mask"] = rng.random((p, p)) < 0.8
    cfg = cm.make_cfg(E, N, W, H, **kw)
    init = synth_init(cfg, seed=seed, n_food_discs=6, food_rmin=2, food_rmax=6, wall_density=0.05)
    _compare_with_oracle(torch_mod, cfg, init, steps=4, seed=seed, jitter_mode="injected")


@pytest.mark.parametrize("seed", range(_BASE + 300, _BASE + 300 + max(32, _CASES // 2)))
def test_random_configuration_library_jitter_no_reads_between_steps(torch_mod, seed):
    """The random configurations driven the way bench.py does: one antsrl_step_update per step with the library's own
    wall jitter and NO state read in between, so that every update that can be deferred into the next step is
    (k_update_move, include/antsrl.h "DEFERRED UPDATE"); outputs of every step and the final state against the oracle,
    which implements the same counter-based jitter."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    from oracle.oracle import Oracle
    from helpers import phero_close
    rng = np.random.default_rng(5000 + seed)
    E, N, W, H, kw = _random_case(rng)
    kw["n_phero"] = 2
    if kw["channels"] is not None:
        kw["channels"] = [(k, a % 2) for k, a in kw["channels"]]
    if rng.random() < 0.5:  # the generator's own layout: the cell-meta path where the perception shape allows it
        kw["channels"] = None
        kw["perception_radius"], kw["mask"] = 3, None
        kw.pop("phero_max_val", None)  # (pheromone is perceived again: max_val is needed)
        if seed % 2 == 0:  # ... and every second of these on the product's hot layout: scaled units, interleaved records in
            # blocks of 2 x 4 cells (KP::tiled needs W even, H a multiple of 4), the update deferred into k_update_move
            W, H = W & ~1, H & ~3
            kw["filt"], kw["phero_mode"] = np.array([[float(rng.choice([0.999, 0.9]))]]), cm.PHERO_AUTO
        elif seed % 4 == 1:  # ... a quarter on the explicit-sweep layout with its {food, META} records in blocks of 4 x 4 cells
            # (KP::ftile needs W and H multiples of 4): a second gather per cell, separate pheromone buffers
            W, H = max(W & ~3, 12), max(H & ~3, 12)
            kw["phero_mode"] = cm.PHERO_EXPLICIT_SWEEP
    # round 4: the shard's global env ids key the library's jitter (AntsCfg.env_id_base) — device and oracle alike —, and a
    # third of the cell-meta cases write padded observation rows (antsrl_set_obs_row_stride)
    kw["env_id_base"] = int(rng.integers(0, 1 << 20)) if rng.random() < 0.7 else 0
    padded = rng.random() < 0.33
    cfg = cm.make_cfg(E, N, W, H, **kw)
    init = synth_init(cfg, seed=seed, n_food_discs=4, food_rmin=1, food_rmax=4, wall_density=0.08)
    env, orc = BatchedAntsEnv(cfg), Oracle(cfg, init)
    if padded and env.query(cm.Q_CELL_META):
        env = BatchedAntsEnv(cfg, obs_row_stride="line")
    env.reset(init)
    prev_dist = _anthill_dist(init, orc.ants_xyt)
    for t in range(7):
        rot = rng.integers(-1, 2, (E, N), dtype=np.int8)
        ph = rng.integers(0, 3, (E, N), dtype=np.int8) if t != 4 else None
        obs, ast, rew, done = env.step_update(rot, ph, None)
        o_obs, o_ast, o_rew, o_done = orc.step(rot, ph)
        g = _cpu(obs)
        for e in range(E):
            check_obs(cfg, g[e], o_obs[e], "seed %d step %d env %d" % (seed, t, e))
        np.testing.assert_array_equal(_cpu(ast), o_ast.astype(np.float32))
        _check_reward(cfg, init, _cpu(rew), o_rew, orc.ants_xyt, prev_dist, "seed %d step %d" % (seed, t))
        prev_dist = _anthill_dist(init, orc.ants_xyt)
        np.testing.assert_array_equal(_cpu(done), o_done)
        orc.update(None)
    assert phero_close(_cpu(env.read_state(cm.S_PHERO)), orc.phero, threshold=cfg.phero_threshold).all()
    np.testing.assert_allclose(_cpu(env.read_state(cm.S_ANTS_XYT)), orc.ants_xyt, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_FOOD)), orc.food)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_ANTHILL_FOOD)), orc.anthill_food)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_EXPLORED)), orc.explored)


# ---- the motion and reward parameters no other random case moves ----------------------------------------------------
# _random_case leaves carry_speed_reduction, backward_speed_reduction, max_rot_speed, reward_threshold and four of
# All_Rewards' five weights at their defaults.  These cases overlay them, from a generator of their own (so _random_case's
# draws, and every other test's, stay what they were), and start a third of the ants on cells with up to 8 food: an ant
# that takes 4 or 5 at carry 0.3 / 0.5 walks backwards from its first step on.
# (seeds 641..672, fixed: chosen on the oracle so that test_motion_cases_contain_what_they_are_for holds — 10 cases with a
#  backward ant-step under a factor other than 1, 5 without exploration; other seeds are not known to reach its floors)
_MOTION_BASE, _MOTION_CASES = 641, 32
_DEG = np.pi / 180


def _motion_case(seed):
    """-> cfg, init, rot[T,E,N], ph[T,E,N] of one case (T = 7 steps; the injected-jitter drive uses its own actions).

    Beyond overlaying the motion and reward parameters on _random_case, two things are forced, as
    test_random_configuration_library_jitter_no_reads_between_steps forces them: two pheromones (pheromone actions need
    exactly two, ants.py:89-96, and so does k_update_move), and in half of the cases the generator's own channel layout with
    radius 3 and at most 1024 ants — the only shape whose update is deferred, so that the move inside k_update_move runs."""
    from antsrl_amd import config as cm
    from antsrl_amd.synth import synth_init
    E, N, W, H, kw = _random_case(np.random.default_rng(7000 + seed))
    rng = np.random.default_rng(9000 + seed)  # the overlay's own generator
    kw["n_phero"] = 2
    if kw["channels"] is not None:
        kw["channels"] = [(k, a % 2) for k, a in kw["channels"]]
    if rng.random() < 0.5:  # the generator's own layout: the cell-meta path, the update deferred into k_update_move
        kw["channels"], kw["perception_radius"], kw["mask"] = None, 3, (None if rng.random() < 0.5 else cm.DEFAULT_MASK)
        kw.pop("phero_max_val", None)
        N = min(N, 1024)
    kw["carry_speed_reduction"] = float(rng.choice([0.05, 0.12, 0.3, 0.5]))
    kw["backward_speed_reduction"] = float(rng.choice([0.5, 0.25, 1.0, 0.0]))
    kw["max_rot_speed"] = float(rng.choice([40 * _DEG, 25 * _DEG, 90 * _DEG, 0.0]))
    kw["reward_threshold"] = float(rng.choice([1.0, 0.35, 0.0, 2.5]))
    pool = [0.0, 0.3, 1.0, 2.0, 7.0]
    for k in ("fct_explore", "fct_food", "fct_anthill", "fct_explore_holding", "fct_headinganthill"):
        kw[k] = float(rng.choice(pool))
    if rng.random() < 0.25:
        kw["fct_explore"] = kw["fct_explore_holding"] = 0.0
    if rng.random() < 0.5:
        kw["reward_kind"] = cm.REWARD_ALL
    kw["env_id_base"] = int(rng.integers(0, 1 << 20)) if rng.random() < 0.7 else 0
    cfg = cm.make_cfg(E, N, W, H, **kw)
    init = synth_init(cfg, seed=seed, n_food_discs=4, food_rmin=1, food_rmax=4, wall_density=0.08)
    init["food"] = (init["food"] * rng.integers(1, 9, init["food"].shape)).astype(np.float32)
    for e in range(E):  # every third ant onto a food cell, anywhere inside it
        fx, fy = np.nonzero(init["food"][e])
        if len(fx):
            idx = np.arange(0, N, 3)
            pick = rng.integers(0, len(fx), len(idx))
            init["ants_xyt"][e, idx, 0] = fx[pick] + rng.uniform(0.05, 0.95, len(idx))
            init["ants_xyt"][e, idx, 1] = fy[pick] + rng.uniform(0.05, 0.95, len(idx))
    # On a grid under 20 cells wide the anthill's radius is 0 and synth_init puts every ant exactly on its centre, an
    # integer point; at 90 degrees a step an ant walks a square and is back there, to the last bit or one off, after four
    # steps, and which cell it then stands in is the device's sincos against the host's.  Such ants start inside the cell.
    xy = init["ants_xyt"][..., :2]
    on_lattice = np.abs(xy - np.round(xy)) < 1e-6
    xy[on_lattice] = np.floor(xy[on_lattice] + 0.5) + rng.uniform(0.05, 0.95, int(on_lattice.sum()))
    xy[..., 0] %= W
    xy[..., 1] %= H
    rot = rng.integers(-1, 2, (7, E, N), dtype=np.int8)
    ph = rng.integers(0, 3, (7, E, N), dtype=np.int8)
    return cfg, init, rot, ph


def _distance_to_lattice(orc):
    xy = orc.ants_xyt[..., :2]
    return float(np.abs(xy - np.round(xy)).min())


def test_motion_cases_contain_what_they_are_for():
    """On the oracle's side, for both drives of the test below: of the 32 cases at least 8 contain a backward ant-step
    that the branch changes (holding * carry > 1 when the step moves the ant, and a backward factor other than 1) and at
    least 4 run All_Rewards without exploration (both explore weights 0: no count, no explored map); and no ant comes
    closer to a cell's edge than the coordinate tolerance, where the device's last bit would choose the cell."""
    from antsrl_amd import config as cm
    from antsrl_amd.synth import random_actions
    from oracle.oracle import Oracle
    from test_gpu_parity import XY_ATOL
    backward, no_explore, nearest = [], [], 1.0
    for seed in range(_MOTION_BASE, _MOTION_BASE + _MOTION_CASES):
        cfg, init, rot, ph = _motion_case(seed)
        # the deferred drive
        orc = Oracle(cfg, init, n_threads=4)
        n = 0
        for t in range(len(rot)):
            o_obs, o_ast, o_rew, o_done = orc.step(rot[t], ph[t] if t != 4 else None, want_obs=False)
            # (a factor of 1 leaves the move what it is without the branch: such a case does not count)
            n += int((o_ast[..., 0] * cfg.carry_speed_reduction > 1).sum()) * (cfg.backward_speed_reduction != 1.0)
            nearest = min(nearest, _distance_to_lattice(orc))
            orc.update(None)
            nearest = min(nearest, _distance_to_lattice(orc))
        if n:
            backward.append(seed)
        if cfg.reward_kind == cm.REWARD_ALL and cfg.fct_explore == 0 and cfg.fct_explore_holding == 0:
            no_explore.append(seed)
            assert not orc.explored.any()
        # the injected-jitter drive, as _compare_with_oracle draws it
        orc = Oracle(cfg, init, n_threads=4)
        r5, p5 = random_actions(cfg, 5, seed)
        rng = np.random.default_rng(seed)
        for t in range(5):
            orc.step(r5[t], p5[t], want_obs=False)
            nearest = min(nearest, _distance_to_lattice(orc))
            orc.update(rng.random((cfg.n_envs, cfg.n_ants)))
            nearest = min(nearest, _distance_to_lattice(orc))
    print("backward:", backward, "no exploration:", no_explore, "nearest to a cell's edge:", nearest)
    assert len(backward) >= 8 and len(no_explore) >= 4
    assert nearest >= XY_ATOL


@pytest.mark.parametrize("seed", range(_MOTION_BASE, _MOTION_BASE + _MOTION_CASES))
def test_random_motion_and_reward_parameters_vs_oracle(torch_mod, seed):
    """Each case twice: step / update with injected wall jitter and the state read after every update
    (_compare_with_oracle: k_move or k_act, k_update_one), then one antsrl_step_update per step with the library's jitter
    and no read in between (the move inside k_update_move wherever the handle defers the update)."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from oracle.oracle import Oracle
    from helpers import phero_close
    cfg, init, rot, ph = _motion_case(seed)
    E = cfg.n_envs
    _compare_with_oracle(torch_mod, cfg, init, steps=5, seed=seed, jitter_mode="injected")
    env, orc = BatchedAntsEnv(cfg), Oracle(cfg, init, n_threads=4)
    env.reset(init)
    prev_dist = _anthill_dist(init, orc.ants_xyt)
    for t in range(len(rot)):
        q = ph[t] if t != 4 else None
        obs, ast, rew, done = env.step_update(rot[t], q, None)
        o_obs, o_ast, o_rew, o_done = orc.step(rot[t], q)
        g = _cpu(obs)
        for e in range(E):
            check_obs(cfg, g[e], o_obs[e], "seed %d step %d env %d" % (seed, t, e))
        np.testing.assert_array_equal(_cpu(ast), o_ast.astype(np.float32))
        _check_reward(cfg, init, _cpu(rew), o_rew, orc.ants_xyt, prev_dist, "seed %d step %d" % (seed, t))
        prev_dist = _anthill_dist(init, orc.ants_xyt)
        np.testing.assert_array_equal(_cpu(done), o_done)
        orc.update(None)
    assert phero_close(_cpu(env.read_state(cm.S_PHERO)), orc.phero, threshold=cfg.phero_threshold).all()
    np.testing.assert_allclose(_cpu(env.read_state(cm.S_ANTS_XYT)), orc.ants_xyt, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_HOLDING)), orc.holding)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_FOOD)), orc.food)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_ANTHILL_FOOD)), orc.anthill_food)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_EXPLORED)), orc.explored)
    np.testing.assert_array_equal(_cpu(env.read_state(cm.S_REWARD_STATE)), orc.reward_state)
