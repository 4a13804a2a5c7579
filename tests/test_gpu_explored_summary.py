"""The explored summary of the cell-meta path (include/antsrl.h, antsrl_set_perceive_path; antsrl_amd/csrc/antsrl_explored.h):
one bit per tile of 8 x 8 cells, "every cell of this tile has been explored", kept in the workspace's "explored_bits" array,
and k_perceive's fast path skipping the record gathers of an ant's masked cells where every tile its patch can touch has
its bit.

1. Bit-identity: three twins — the default path with a refresh forced every 4 steps, ANTSRL_PERCEIVE_FAST_NOSKIP and
   ANTSRL_PERCEIVE_GENERIC — agree bit for bit at every step on observation, reward, agent_state, done, the explored map and
   the ant state, from a reset until the map is explored; the float32 rows are held to the CPU oracle.
2. Soundness and completeness of the bits after each forced refresh, against ANTSRL_S_EXPLORED.
3. Engagement: with a forged all-ones summary on a fresh map the skipping handle counts and marks 37 cells per ant, its
   FAST_NOSKIP twin 49 — the kernel reads the summary, and a skipping lane neither counts nor marks.
4. Lifecycle: cleared by reset / generate / auto-reset, first set behind observation 256, the query (0 under GENERIC and
   FAST_NOSKIP, without a mask, without a reward that counts explored cells, without the rock channel), k_act untouched.
5. The stamp re-base (every 16 381 observations) is crossed with set bits.

The tests read the bits themselves, from a state block they own (antsrl_workspace_map).
Shapes: 32 x 32 and 64 x 32 cells (more than one tile per axis), 16 x 16 (the box always covers the whole grid), E = 3, N = 40
(a ragged last wave), with and without a rock.  The library keeps the summary where the rock channel is perceived (the
instantiations of k_perceive in which the skip pays: include/antsrl.h), so the cases with a rock run the skip and the cases
without one pin that nothing is kept or consumed there.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_perceive_fastpath import _assert_oracle, _border_init, _cpu

pytestmark = pytest.mark.gpu

E, N = 3, 40
FORCE_EVERY = 4


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _bits_view(torch, env, state):
    """The int32 view [E][words] of the handle's "explored_bits" array inside the state block `state` the test owns."""
    from antsrl_amd import _lib
    n = C.c_int32()
    _lib.check(env.lib.antsrl_workspace_map(C.byref(env.cfg), 1, None, 0, C.byref(n)), "workspace_map")
    arr = (_lib.AntsWsArray * n.value)()
    _lib.check(env.lib.antsrl_workspace_map(C.byref(env.cfg), 1, arr, n.value, C.byref(n)), "workspace_map")
    ent = [a for a in arr if a.name == b"explored_bits"]
    assert len(ent) == 1 and ent[0].block == 0, "explored_bits lives in the state block"
    words = (env.cfg.w * env.cfg.h + 31) // 32
    assert ent[0].bytes >= 4 * env.cfg.n_envs * words
    return state[ent[0].offset:ent[0].offset + 4 * env.cfg.n_envs * words].view(torch.int32).view(env.cfg.n_envs, words)


def _env(torch, cfg, path, dtype=None):
    """-> (env on blocks the test owns, the bits view).  `path`: config.PERCEIVE_*."""
    from antsrl_amd.batched import BatchedAntsEnv
    env = BatchedAntsEnv(cfg, "cuda:0", obs_dtype=dtype or torch.float32)
    rec = torch.empty(env.record_bytes + 256, dtype=torch.uint8, device=env.device)
    st = torch.zeros(env.state_bytes + 256, dtype=torch.uint8, device=env.device)
    off = (-st.data_ptr()) % 256
    st = st[off:off + env.state_bytes]
    env._make_handle(rec, st)
    env.set_perceive_path(path)
    return env, _bits_view(torch, env, st)


def _tile_bits(cfg, bits):
    """bits [E][words] (numpy int32) -> bool [E][W/8][H/8], and whether any bit past the tiles is set."""
    nt = (cfg.w // 8) * (cfg.h // 8)
    flat = np.unpackbits(bits.view(np.uint8).reshape(cfg.n_envs, -1), axis=1, bitorder="little")
    return flat[:, :nt].astype(bool).reshape(cfg.n_envs, cfg.w // 8, cfg.h // 8), bool(flat[:, nt:].any())


def _tiles_full(cfg, explored):
    return explored.reshape(cfg.n_envs, cfg.w // 8, 8, cfg.h // 8, 8).astype(bool).all(axis=(2, 4))


STATE = ("S_EXPLORED", "S_ANTS_XYT", "S_PREV_XY", "S_HOLDING", "S_MANDIBLES", "S_FOOD", "S_REWARD_STATE")


@functools.lru_cache(maxsize=None)
def _case(W, H, rocks, steps):
    from antsrl_amd import config as cm
    from antsrl_amd.synth import random_actions
    cfg = cm.make_cfg(E, N, W, H, n_rocks=rocks, deposit_strength=256.0, act_path=cm.ACT_CELL_META)
    init = _border_init(cfg, seed=31 + W + 3 * H + rocks, wall_density=0.04)
    rot, ph = random_actions(cfg, steps, seed=W + rocks)
    return cfg, init, rot, ph


@functools.lru_cache(maxsize=None)
def _oracle_steps(W, H, rocks, steps):
    from oracle.oracle import Oracle
    cfg, init, rot, ph = _case(W, H, rocks, steps)
    orc = Oracle(cfg, init, n_threads=4)
    out = []
    for t in range(steps):
        o_obs, o_ast, o_rew, _ = orc.step(rot[t], ph[t])
        out.append((np.array(o_obs), np.array(o_ast), np.array(o_rew)))
        orc.update(None)
    return out, np.array(orc.explored), np.array(orc.food)


# steps: enough for 40 ants to have seen every cell (the oracle's maps are full at steps 14 / 20 / 52 / 49 / 1), and then
# some with every ant skipping
@pytest.mark.parametrize("rows", ["float32", "bfloat16", "act_only"])
@pytest.mark.parametrize("W,H,rocks,steps", [(32, 32, 0, 40), (32, 32, 1, 40), (64, 32, 0, 72), (64, 32, 1, 72), (16, 16, 1, 24)])
def test_twins_agree_and_bits_are_sound_and_complete(torch_mod, W, H, rocks, steps, rows):
    torch = torch_mod
    from antsrl_amd import config as cm
    cfg, init, rot, ph = _case(W, H, rocks, steps)
    dtype = torch.float32 if rows == "float32" else torch.bfloat16
    want_obs = rows != "act_only"
    twins = [_env(torch, cfg, p, dtype) for p in (cm.PERCEIVE_AUTO, cm.PERCEIVE_FAST_NOSKIP, cm.PERCEIVE_GENERIC)]
    (auto, bits), (noskip, bits_ns), (gen, bits_gen) = twins
    kept = rocks > 0
    assert [e.query(cm.Q_EXPLORED_SUMMARY) for e, _ in twins] == [int(kept), 0, 0]
    assert [e.query(cm.Q_PERCEIVE_FAST) for e, _ in twins] == [1, 1, 0]
    for env, _ in twins:
        env.reset(init)
    got = []
    skipped_steps = 0  # steps taken with every tile's bit set: every ant of the default twin skips
    for t in range(steps):
        all_set = bool(_tile_bits(cfg, bits.cpu().numpy())[0].all())
        skipped_steps += all_set
        outs = []
        for env, _ in twins:
            obs, ast, rew, done = env.step(rot[t], ph[t], want_obs=want_obs)
            outs.append((obs.clone() if want_obs else None, ast.clone(), rew.clone(), done.clone()))
            env.update(None)
        for name, k in (("observation", 0), ("agent_state", 1), ("reward", 2), ("done", 3)):
            if outs[0][k] is None:
                continue
            for other, who in ((1, "FAST_NOSKIP"), (2, "GENERIC")):
                assert torch.equal(outs[0][k], outs[other][k]), "step %d %s: AUTO differs from %s" % (t, name, who)
        for sel in STATE:
            a = auto.read_state(getattr(cm, sel))
            assert torch.equal(a, noskip.read_state(getattr(cm, sel))), "step %d state %s: AUTO / FAST_NOSKIP" % (t, sel)
            assert torch.equal(a, gen.read_state(getattr(cm, sel))), "step %d state %s: AUTO / GENERIC" % (t, sel)
        if rows == "float32":
            got.append(tuple(_cpu(x).copy() for x in outs[0][:3]))
        if t % FORCE_EVERY == FORCE_EVERY - 1:
            for env, _ in twins:  # (a no-op on the two that keep no summary)
                env.refresh_explored_summary()
            tiles, stray = _tile_bits(cfg, bits.cpu().numpy())
            full = _tiles_full(cfg, _cpu(auto.read_state(cm.S_EXPLORED)))
            assert not stray, "step %d: a bit past the first (W/8)(H/8)" % t
            assert not (tiles & ~full).any(), "step %d: a set bit over a tile with an unexplored cell" % t
            assert not kept or not (full & ~tiles).any(), "step %d: a fully explored tile without its bit" % t
            assert kept or not tiles.any(), "step %d: no summary is kept without the rock channel" % t
            assert not bits_ns.any() and not bits_gen.any(), "a handle that keeps no summary wrote one"
    assert _cpu(auto.read_state(cm.S_EXPLORED)).all(), "the case is built so that the map ends fully explored"
    assert not kept or skipped_steps >= 8, "the case is built so that steps run with every ant skipping (%d did)" % skipped_steps
    if rows == "float32":
        o_steps, o_expl, o_food = _oracle_steps(W, H, rocks, steps)
        _assert_oracle(cfg, (got, _cpu(auto.read_state(cm.S_EXPLORED)), _cpu(auto.read_state(cm.S_FOOD))), (o_steps, o_expl, o_food), "AUTO")


@pytest.mark.parametrize("W,H", [(32, 32), (64, 32), (16, 16)])
def test_a_forged_summary_shows_the_skip(torch_mod, W, H):
    """Nothing is explored, yet the test sets every tile's bit: the skipping handle's masked lanes count nothing and mark
    nothing (reward 37 / 10 per ant, the explored map = the unmasked perceived cells); FAST_NOSKIP counts and marks all 49."""
    torch = torch_mod
    from antsrl_amd import config as cm
    cfg, init, _, _ = _case(W, H, 1, 40)
    assert cfg.reward_kind == cm.REWARD_EXPLORATION and int(cm.mask_array(cfg).sum()) == 37
    (auto, bits), (noskip, _) = _env(torch, cfg, cm.PERCEIVE_AUTO), _env(torch, cfg, cm.PERCEIVE_FAST_NOSKIP)
    for env in (auto, noskip):
        env.reset(init)
        env.refresh_explored_summary()  # (the kernel consults the summary from an episode's first refresh on; it finds no tile)
    assert not bits.any()
    nt = (W // 8) * (H // 8)
    forged = np.zeros(bits.shape, np.uint32)
    for t in range(nt):
        forged[:, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    bits.copy_(torch.from_numpy(forged.view(np.int32)).to(bits.device))
    torch.cuda.synchronize()
    _, _, r_a = auto.observe()
    _, _, r_n = noskip.observe()
    assert torch.equal(r_a, torch.full_like(r_a, np.float32(37 / 10.0)))
    assert torch.equal(r_n, torch.full_like(r_n, np.float32(49 / 10.0)))
    seen = auto.perceptive_field()  # the cells some ant perceives, masked cells not counted
    assert torch.equal(auto.read_state(cm.S_EXPLORED).bool(), seen), "a skipping lane marked its masked cell (or a needed one did not)"
    marked = noskip.read_state(cm.S_EXPLORED).bool()
    assert bool((marked | ~seen).all()) and int(marked.sum()) > int(seen.sum())
    assert torch.equal(auto.obs, noskip.obs)  # (masked cells read -1 either way)


def test_lifecycle_query_and_k_act(torch_mod):
    torch = torch_mod
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions
    cfg = cm.make_cfg(E, N, 32, 32, n_rocks=1, deposit_strength=256.0, act_path=cm.ACT_CELL_META, max_time=270)
    env, bits = _env(torch, cfg, cm.PERCEIVE_AUTO)
    assert env.query(cm.Q_EXPLORED_SUMMARY) == 1
    rot, ph = random_actions(cfg, 280, seed=4)
    env.generate(cm.make_gen(wall_density=0.02, n_food_discs=2, food_rmin=1, food_rmax=2, auto_reset=True), episode_seed=3)
    for t in range(255):
        env.step_update(rot[t], ph[t])
    assert not bits.any(), "no refresh before observation 256"
    env.step_update(rot[255], ph[255])
    assert bits.any(), "the first refresh comes behind observation 256"
    tiles, stray = _tile_bits(cfg, bits.cpu().numpy())
    assert not stray and not (tiles & ~_tiles_full(cfg, _cpu(env.read_state(cm.S_EXPLORED)))).any()
    done = False
    for t in range(256, 280):  # the episode ends at max_time: auto-reset
        done = bool(env.step_update(rot[t], ph[t])[3].all())
        if done:
            break
    assert done and not bits.any(), "an auto-reset clears the summary"
    for t in range(256):  # ... and the cadence restarts with the episode
        assert t % 32 or not bits.any()
        env.step_update(rot[t], ph[t])
    assert bits.any()
    env.generate(cm.make_gen(wall_density=0.02, n_food_discs=2, food_rmin=1, food_rmax=2), episode_seed=5)
    assert not bits.any(), "antsrl_generate clears the summary"
    for t in range(256):
        env.step_update(rot[t], ph[t])
    assert bits.any()
    env.reset(_border_init(cfg, seed=2))
    assert not bits.any(), "antsrl_reset clears the summary"
    # the query: the generic kernel, the fast kernel without the skip, no mask, a reward that counts no explored cells
    env.set_perceive_path(cm.PERCEIVE_GENERIC)
    assert env.query(cm.Q_EXPLORED_SUMMARY) == 0
    env.set_perceive_path(cm.PERCEIVE_FAST_NOSKIP)
    assert env.query(cm.Q_EXPLORED_SUMMARY) == 0 and env.query(cm.Q_PERCEIVE_FAST) == 1
    env.set_perceive_path(cm.PERCEIVE_AUTO)
    assert env.query(cm.Q_EXPLORED_SUMMARY) == 1
    for kw in (dict(n_rocks=1, mask=None), dict(n_rocks=1, reward_kind=cm.REWARD_FOOD), dict(n_rocks=0)):
        other = BatchedAntsEnv(cm.make_cfg(E, N, 32, 32, act_path=cm.ACT_CELL_META, **kw), "cuda:0")
        assert other.query(cm.Q_CELL_META) == 1 and other.query(cm.Q_EXPLORED_SUMMARY) == 0
    # k_act keeps the array as its explored MAP: bit x * H + y
    odd = [(cm.CH_FOOD, 0), (cm.CH_ANTS, 0), (cm.CH_PHERO, 0), (cm.CH_PHERO, 1), (cm.CH_WALLS, 0)]
    cfg_a = cm.make_cfg(E, N, 32, 32, channels=odd)
    act, bits_a = _env(torch, cfg_a, cm.PERCEIVE_AUTO)
    assert act.query(cm.Q_CELL_META) == 0 and act.query(cm.Q_EXPLORED_SUMMARY) == 0
    act.reset(_border_init(cfg_a, seed=2))
    for t in range(6):
        act.step_update(rot[t], ph[t])
    act.refresh_explored_summary()  # (nothing to do, and nothing done)
    packed = np.unpackbits(bits_a.cpu().numpy().view(np.uint8).reshape(E, -1), axis=1, bitorder="little")[:, :32 * 32]
    np.testing.assert_array_equal(packed.reshape(E, 32, 32), _cpu(act.read_state(cm.S_EXPLORED)))


def test_set_bits_survive_the_stamp_rebase(torch_mod):
    """The explored stamps are re-based every 16 381 observations (explored cells -> stamp 0).  Crossed here with every bit
    set, by observations that move nobody; the twins then step on, bit for bit."""
    torch = torch_mod
    from antsrl_amd import config as cm
    cfg, init, rot, ph = _case(16, 16, 1, 40)
    (auto, bits), (gen, _) = _env(torch, cfg, cm.PERCEIVE_AUTO), _env(torch, cfg, cm.PERCEIVE_GENERIC)
    for env in (auto, gen):
        env.reset(init)
        for t in range(32):
            env.step_update(rot[t], ph[t])
    auto.refresh_explored_summary()
    assert _tile_bits(cfg, bits.cpu().numpy())[0].all(), "the case is built so that the 16 x 16 map is explored by step 32"
    for env in (auto, gen):
        for _ in range(16381 - 32 + 2):  # past the re-base, whichever observation triggers it
            env.observe(want_obs=False)
    assert _tile_bits(cfg, bits.cpu().numpy())[0].all()
    for t in range(32, 40):
        outs = [[x.clone() for x in env.step_update(rot[t], ph[t])] for env in (auto, gen)]
        for a, b, name in zip(outs[0], outs[1], ("observation", "agent_state", "reward", "done")):
            assert torch.equal(a, b), "step %d behind the re-base: %s" % (t, name)
    for sel in STATE:
        assert torch.equal(auto.read_state(getattr(cm, sel)), gen.read_state(getattr(cm, sel))), sel
    assert _cpu(auto.read_state(cm.S_EXPLORED)).all()
