"""k_perceive's fast path (power-of-two grid, interleaved records in 2 x 4-cell blocks, a perception mask) against its generic
path and against the CPU oracle.

The two paths differ in how a perceived cell's record is found (grid wrap, record slot), in whether the gather address goes
through a lane permute (only when some lane borrows another lane's address) and in where a wave's rock masks live; no
arithmetic differs, so every output is compared bit for bit.  The generic path is pinned on a handle with
antsrl_set_perceive_path; antsrl_query(ANTSRL_Q_PERCEIVE_FAST) tells which one a handle runs.

Compared: observation, agent_state, reward of every step, and the explored map and the food grid read back after the last
update (antsrl_read_state).  The state read-out has no selector for the presence stamps: they are compared through the
observation's Ants channel, which is nothing but `stamp == this observation`.

Grids are 32 x 32 (36 x 40 / 33 x 32 for the fallback): ants start on the borders and in all four corners, so patches wrap on
both axes from the first observation on.
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import check_obs

pytestmark = pytest.mark.gpu

STEPS = 6


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _cpu(t):
    return t.detach().float().cpu().numpy() if t.dtype.is_floating_point else t.detach().cpu().numpy()


def _border_init(cfg, seed, **kw):
    """synth_init with the first ants moved onto the borders and into the four corners (headings left as drawn)."""
    from antsrl_amd.synth import synth_init
    kw.setdefault("n_food_discs", 6)
    kw.setdefault("food_rmin", 2)
    kw.setdefault("food_rmax", 4)
    kw.setdefault("wall_density", 0.08)
    init = synth_init(cfg, seed=seed, **kw)
    W, H = cfg.w, cfg.h
    spots = [(0.5, 0.5), (W - 0.5, 0.5), (0.5, H - 0.5), (W - 0.5, H - 0.5), (0.25, H / 2), (W - 0.25, H / 3),
             (W / 2, 0.25), (W / 3, H - 0.25), (1.5, 1.5), (W - 1.5, H - 1.5)]
    for e in range(cfg.n_envs):
        for i, (x, y) in enumerate(spots[:cfg.n_ants]):
            a = (i + 3 * e) % cfg.n_ants  # (a different set of ants in every environment: first and last waves alike)
            init["ants_xyt"][e, a, 0] = x
            init["ants_xyt"][e, a, 1] = y
    return init


def _run_device(torch, cfg, init, rot, ph, generic, dtype=None, expect_fast=None):
    """-> per-step (obs, agent_state, reward) as numpy, and the explored / food maps after the last update."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    env = BatchedAntsEnv(cfg, "cuda:0", obs_dtype=dtype or torch.float32)
    assert env.query(cm.Q_CELL_META) == 1
    if generic:
        env.set_perceive_path(cm.PERCEIVE_GENERIC)
        assert env.query(cm.Q_PERCEIVE_FAST) == 0
    elif expect_fast is not None:
        assert env.query(cm.Q_PERCEIVE_FAST) == int(expect_fast)
    env.reset(init)
    steps = []
    for t in range(rot.shape[0]):
        obs, ast, rew, done = env.step(rot[t], ph[t])
        steps.append((_cpu(obs).copy(), _cpu(ast).copy(), _cpu(rew).copy()))
        env.update(None)
    return steps, _cpu(env.read_state(cm.S_EXPLORED)).copy(), _cpu(env.read_state(cm.S_FOOD)).copy()


def _run_oracle(cfg, init, rot, ph):
    from oracle.oracle import Oracle
    orc = Oracle(cfg, init, n_threads=4)
    steps = []
    for t in range(rot.shape[0]):
        o_obs, o_ast, o_rew, _ = orc.step(rot[t], ph[t])
        steps.append((np.array(o_obs), np.array(o_ast), np.array(o_rew)))
        orc.update(None)
    return steps, np.array(orc.explored), np.array(orc.food)


def _assert_same(a, b, ctx):
    (sa, ea, fa), (sb, eb, fb) = a, b
    for t, (x, y) in enumerate(zip(sa, sb)):
        for name, u, v in zip(("observation", "agent_state", "reward"), x, y):
            np.testing.assert_array_equal(u, v, err_msg="%s step %d %s" % (ctx, t, name))
    np.testing.assert_array_equal(ea, eb, err_msg=ctx + " explored")  # (the stamps k_perceive writes)
    np.testing.assert_array_equal(fa, fb, err_msg=ctx + " food")


def _assert_oracle(cfg, got, want, ctx):
    (sg, eg, fg), (sw, ew, fw) = got, want
    for t, ((obs, ast, rew), (o_obs, o_ast, o_rew)) in enumerate(zip(sg, sw)):
        for e in range(cfg.n_envs):
            check_obs(cfg, obs[e], o_obs[e], "%s step %d env %d" % (ctx, t, e))
        np.testing.assert_array_equal(ast, o_ast.astype(np.float32), err_msg="%s step %d agent_state" % (ctx, t))
        np.testing.assert_array_equal(rew, o_rew.astype(np.float32), err_msg="%s step %d reward" % (ctx, t))
    np.testing.assert_array_equal(eg, ew, err_msg=ctx + " explored")
    np.testing.assert_array_equal(fg, fw, err_msg=ctx + " food")


@functools.lru_cache(maxsize=None)
def _case(E, N, rocks):
    from antsrl_amd import config as cm
    from antsrl_amd.synth import random_actions
    cfg = cm.make_cfg(E, N, 32, 32, n_rocks=rocks, deposit_strength=256.0, act_path=cm.ACT_CELL_META)
    init = _border_init(cfg, seed=100 + 7 * E + N + rocks)
    rot, ph = random_actions(cfg, STEPS, seed=E + N)
    return cfg, init, rot, ph, _run_oracle(cfg, init, rot, ph)


# E = 3 / 8: the two branches of the workgroup -> environment map; N = 33 / 40: a last workgroup of one ant and three empty
# waves / whole workgroups only (the batch is small, so a wave takes two ants: N = 33 ends on an odd tail row)
@pytest.mark.parametrize("rocks", [0, 3])
@pytest.mark.parametrize("N", [33, 40])
@pytest.mark.parametrize("E", [3, 8])
def test_fast_equals_generic_bit_for_bit(torch_mod, E, N, rocks):
    torch = torch_mod
    cfg, init, rot, ph, want = _case(E, N, rocks)
    fast = _run_device(torch, cfg, init, rot, ph, generic=False, expect_fast=True)
    gen = _run_device(torch, cfg, init, rot, ph, generic=True)
    _assert_same(fast, gen, "float32 fast / generic")
    _assert_oracle(cfg, fast, want, "fast")
    _assert_oracle(cfg, gen, want, "generic")
    fast16 = _run_device(torch, cfg, init, rot, ph, generic=False, dtype=torch.bfloat16, expect_fast=True)
    gen16 = _run_device(torch, cfg, init, rot, ph, generic=True, dtype=torch.bfloat16)
    _assert_same(fast16, gen16, "bfloat16 fast / generic")
    # bfloat16 observations are the float32 ones rounded to nearest even (include/antsrl.h): through the float32 run, the
    # oracle pins them too
    for t in range(STEPS):
        r16 = torch.from_numpy(fast[0][t][0]).to(torch.bfloat16).float().numpy()
        np.testing.assert_array_equal(fast16[0][t][0], r16, err_msg="bfloat16 step %d" % t)
        np.testing.assert_array_equal(fast16[0][t][2], fast[0][t][2], err_msg="bfloat16 reward step %d" % t)


@pytest.mark.parametrize("W,H", [(36, 40), (33, 32)], ids=["not_pow2", "odd_w_row_major"])
def test_dispatch_falls_back_to_generic(torch_mod, W, H):
    from antsrl_amd import config as cm
    from antsrl_amd.synth import random_actions
    cfg = cm.make_cfg(3, 33, W, H, n_rocks=2, deposit_strength=256.0, act_path=cm.ACT_CELL_META)
    init = _border_init(cfg, seed=W + H)
    rot, ph = random_actions(cfg, STEPS, seed=W)
    got = _run_device(torch_mod, cfg, init, rot, ph, generic=False, expect_fast=False)
    _assert_oracle(cfg, got, _run_oracle(cfg, init, rot, ph), "%dx%d" % (W, H))


# exploration reward + mask: every lane's record is needed (the explored count ignores the mask) — no permute;
# food reward + mask: a masked lane borrows the address of the wave's first needed lane — the permute stays;
# no mask: every lane owns its gather (and the launch takes the generic kernel: the fast path wants a mask)
@pytest.mark.parametrize("reward,masked,fast", [("exploration", True, True), ("food", True, True), ("food", False, False)],
                         ids=["explore_mask_skips", "food_mask_permutes", "no_mask_owns"])
def test_permute_skip_matches_oracle(torch_mod, reward, masked, fast):
    from antsrl_amd import config as cm
    from antsrl_amd.synth import random_actions
    kw = {} if masked else dict(mask=None)
    cfg = cm.make_cfg(3, 40, 32, 32, n_rocks=2, deposit_strength=256.0, act_path=cm.ACT_CELL_META,
                      reward_kind=cm.REWARD_EXPLORATION if reward == "exploration" else cm.REWARD_FOOD, **kw)
    init = _border_init(cfg, seed=55)
    rot, ph = random_actions(cfg, 8, seed=9)
    want = _run_oracle(cfg, init, rot, ph)
    got = _run_device(torch_mod, cfg, init, rot, ph, generic=False, expect_fast=fast)
    _assert_oracle(cfg, got, want, reward)
    _assert_same(got, _run_device(torch_mod, cfg, init, rot, ph, generic=True), reward + " fast / generic")


def test_rock_masks_per_wave(torch_mod):
    """Environment 0: a rock within reach of the patches of ant 0 and ant 7 — the first and the last ant of one wave of eight —
    and of no other ant: every other wave of that environment runs the loop that holds no rock test.  The rock channel
    (and everything else) matches the oracle cell for cell."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    E, N, W, H = 64, 512, 64, 64  # (the smallest batch at which a wave takes eight ants: ANTSRL_Q_PERCEIVE_RUN)
    cfg = cm.make_cfg(E, N, W, H, n_rocks=3, deposit_strength=256.0, act_path=cm.ACT_CELL_META)
    probe = BatchedAntsEnv(cfg, "cuda:0")
    assert probe.query(cm.Q_PERCEIVE_RUN) == 8 and probe.query(cm.Q_PERCEIVE_FAST) == 1
    del probe
    init = synth_init(cfg, seed=5, n_food_discs=6, food_rmin=2, food_rmax=4)
    rng = np.random.default_rng(3)
    xy = init["ants_xyt"][0]
    xy[:, 0] = 40.0 + 8.0 * rng.random(N)  # everybody far from the rocks and from the borders ...
    xy[:, 1] = 40.0 + 8.0 * rng.random(N)
    xy[0, :2] = (20.5, 18.5)               # ... but ants 0 and 7, beside rock 0
    xy[7, :2] = (23.5, 22.5)
    init["rocks"][0, :, :3] = [(21.0, 20.0, 5.0), (52.0, 14.0, 5.0), (14.0, 52.0, 5.0)]
    steps = 6
    rot, ph = random_actions(cfg, steps, seed=2)
    want = _run_oracle(cfg, init, rot, ph)
    got = _run_device(torch_mod, cfg, init, rot, ph, generic=False, expect_fast=True)
    k_rock = cfg.n_channels - 1
    assert cfg.channel_kind[k_rock] == cm.CH_ROCKS
    seen = [False, False]
    for t in range(steps):
        g, w = got[0][t][0][0, ..., k_rock], want[0][t][0][0, ..., k_rock]
        np.testing.assert_array_equal(g, w.astype(np.float32), err_msg="rock channel, step %d" % t)
        seen[0] |= bool((w[0] == 1).any())
        seen[1] |= bool((w[7] == 1).any())
        assert not (w[8:] == 1).any() and not (w[1:7] == 1).any(), "the case is built so that only ants 0 and 7 see a rock"
    assert all(seen), "ants 0 and 7 must see the rock"
    _assert_oracle(cfg, got, want, "rocks")
