"""Checkpoint, restore and fork on the device (include/antsrl.h "CHECKPOINT", antsrl_amd/checkpoint.py).
Every comparison is exact (torch.equal): a restored or forked environment continues bit for bit.

Shapes: (a) E = 5, N = 33, 64 x 64 with walls, food and 2 rocks — 33-byte `mandibles` rows, which no 16-byte access can
copy between environments an odd distance apart; (b) three pheromones (separate scaled buffers); (c) a 3 x 3 diffusing
filter (the ping-pong pair, `cur` matters); (d) 60 x 44 cells, no power of two; (e) the single-kernel path; (f) E = 1,
N = 5, no rocks; (g) bfloat16 observations.

CONTINUATION.  A runs 37 step_updates (library jitter, deferred update where the path has one), is checkpointed, runs 45
more; a fresh B — the other workspace split, its workspace filled with 0xA5, reset to ANOTHER episode — restores the
checkpoint (through a file) and runs the same 45 actions; then A restores it into itself and runs them a third time.
Where the handle keeps an explored summary (shapes a and g) 200 bare observations come first, so that the summary's
first refresh (behind observation 256) falls between the save (observation 238) and the end (283): it is crossed.  NOT crossed, at any shape: the
scaled units' re-base (`sweeps`: once 0.999^sweeps < 1e-20, some 46 000 updates) and the explored stamps' re-base (every
16 381 observations).  Besides the outputs of every step and every read_state selector at the end, a checkpoint taken
from A and from B at the end must be equal byte for byte, block and blob: that covers what no selector shows (the summary's
bits, its cadence, the frames, the generator's tables).

FORK.  fork([1, 1, 3], [0, 4, 2]): odd and even distances, one source fanned out.  GUARD: every byte of a padded
checkpoint block and of the whole workspace (pattern-filled before the reset) that the copy must not write is unchanged.

THE LOOP.  Each of the four device agents: 24 rollout_steps, checkpoint + training_state through files, 24 more; a fresh env
and agent restore both and repeat them.  max_time = 30, so the episode's end — done, the target's sync — lies behind the save.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _diffuse3():
    f3 = np.ones((3, 3)) * 0.02
    f3[1, 1] = 1 - 8 * 0.02
    return f3 * (1 - 0.001)


def _shapes():
    from antsrl_amd import config as cm
    base = dict(n_rocks=2, deposit_strength=256.0)
    return {
        "a_base": ((5, 33, 64, 64), base, {}),
        "b_three_phero": ((5, 33, 64, 64), dict(base, n_phero=3), {}),
        "c_diffuse3x3": ((5, 33, 64, 64), dict(base, filt=_diffuse3()), {}),
        "d_60x44": ((5, 33, 60, 44), base, {}),
        "e_single_kernel": ((5, 33, 64, 64), dict(base, act_path=cm.ACT_SINGLE_KERNEL), {}),
        "f_one_env": ((1, 5, 64, 64), dict(deposit_strength=256.0), {}),
        "g_bf16": ((5, 33, 64, 64), base, dict(bf16=True)),
    }


SHAPE_NAMES = ("a_base", "b_three_phero", "c_diffuse3x3", "d_60x44", "e_single_kernel", "f_one_env", "g_bf16")
SUMMARY_KEPT = ("a_base", "g_bf16")
PRE, POST, PRE_OBSERVES = 37, 45, 200


def _make(name, split=True, seed=3, wall_density=0.05, fill=None, **cfg_kw):
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    dims, kw, opt = _shapes()[name]
    cfg = cm.make_cfg(*dims, **dict(kw, **cfg_kw))
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16 if opt.get("bf16") else torch.float32, split_workspace=split)
    if fill is not None:
        env._ws.fill_(fill)
        if env._state is not None:
            env._state.fill_(fill)
    env.reset(synth_init(cfg, seed=seed, wall_density=wall_density, n_food_discs=6, food_rmin=3, food_rmax=6))
    return env


def _actions(cfg, steps, seed):
    """rotation in {-1, 0, 1} and pheromone in {0, 1, 2} (None unless there are exactly two channels: ants.py:89-96)."""
    import torch
    rng = np.random.default_rng(seed)
    rot = torch.as_tensor(rng.integers(-1, 2, (steps, cfg.n_envs, cfg.n_ants)).astype(np.int8)).cuda()
    ph = torch.as_tensor(rng.integers(0, 3, (steps, cfg.n_envs, cfg.n_ants)).astype(np.int8)).cuda()
    return rot, (ph if cfg.n_phero == 2 else None)


def _outputs(env):
    return tuple(t.clone() for t in (env.obs, env.agent_state, env.reward, env.done))


def _run(env, rot, ph, jitter=None):
    out = []
    for t in range(rot.shape[0]):
        env.step_update(rot[t], None if ph is None else ph[t], None if jitter is None else jitter[t])
        out.append(_outputs(env))
    return out


def _read_all(env):
    from antsrl_amd import config as cm
    from antsrl_amd.batched import _STATE_ARRAYS
    return {w: env.read_state(w) for w in sorted(_STATE_ARRAYS)
            if not (cm.S_PHERO_C0 <= w <= cm.S_PHERO_C3 and w - cm.S_PHERO_C0 >= env.cfg.n_phero)}


def _same_steps(a, b, what):
    import torch
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k, u, v in zip(("obs", "agent_state", "reward", "done"), x, y):
            assert torch.equal(u, v), "%s: %s differs at step %d" % (what, k, t)


def _same_state(a, b, what):
    import torch
    assert a.keys() == b.keys()
    for w in a:
        assert torch.equal(a[w], b[w]), "%s: read_state selector %d differs" % (what, w)


def _same_checkpoint(a, b, what):
    import torch
    assert a.blob == b.blob, "%s: the blobs differ" % what
    arrays_b = b.arrays()
    bad = [n for n, v in a.arrays().items() if not torch.equal(v, arrays_b[n])]
    assert not bad, "%s: the blocks differ in %s" % (what, bad)  # (the bytes between two arrays are nobody's)
    for k in ("obs", "agent_state", "reward", "done"):
        assert torch.equal(getattr(a, k), getattr(b, k)), "%s: %s differs" % (what, k)


def _summary_fields(ck):
    """(sum_obs, sum_live) of a format-1 blob: behind magic, version, size (16 bytes) and the AntsCfg come five 32-bit
    fields, sum_obs the last of them, then the flags, sum_live the sixth (antsrl_checkpoint.h)."""
    from antsrl_amd.config import AntsCfg
    at = 16 + C.sizeof(AntsCfg)
    return int.from_bytes(ck.blob[at + 16:at + 20], "little"), ck.blob[at + 20 + 5]


@functools.lru_cache(maxsize=None)
def _continuation(name, tmp):
    """The three runs of one shape (the module docstring); computed once, shared by the tests below."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.checkpoint import EnvCheckpoint
    A = _make(name, split=True)
    cfg = A.cfg
    kept = bool(A.query(cm.Q_EXPLORED_SUMMARY))
    assert kept == (name in SUMMARY_KEPT), (name, kept)
    A.observe()
    if kept:
        for _ in range(PRE_OBSERVES):
            A.observe()
    rot, ph = _actions(cfg, PRE + POST, seed=11)
    deferred = bool(A.query(cm.Q_DEFERRED_UPDATE))
    _run(A, rot[:PRE], None if ph is None else ph[:PRE])
    ck = A.checkpoint()
    path = "%s/%s.ckpt" % (tmp, name)
    ck.save(path)
    from_file = EnvCheckpoint.load(path, A.device)
    post = (rot[PRE:], None if ph is None else ph[PRE:])
    first = _run(A, *post)
    end_a, ck_a = _read_all(A), A.checkpoint()
    B = _make(name, split=False, seed=19, fill=0xA5)  # the other split, a dirty workspace, another episode
    B.restore(from_file)
    second = _run(B, *post)
    end_b, ck_b = _read_all(B), B.checkpoint()
    A.restore(ck)  # into the handle it came from, after that handle has run on
    third = _run(A, *post)
    end_a3, ck_a3 = _read_all(A), A.checkpoint()
    torch.cuda.synchronize()
    return SimpleNamespace(ck=ck, from_file=from_file, first=first, second=second, third=third, end=(end_a, end_b, end_a3),
                           end_ck=(ck_a, ck_b, ck_a3), kept=kept, deferred=deferred)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ckpt"))


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_a_restored_handle_continues_bit_for_bit(torch_mod, tmp, name):
    r = _continuation(name, tmp)
    # (the update is deferred wherever the cell-meta path runs: not with three pheromones, not on the single-kernel path)
    assert r.deferred == (name not in ("b_three_phero", "e_single_kernel"))
    _same_steps(r.first, r.second, "fresh handle, other split")
    _same_state(r.end[0], r.end[1], "fresh handle, other split")
    _same_checkpoint(r.end_ck[0], r.end_ck[1], "fresh handle, other split")
    if r.kept:  # the summary's first refresh was crossed behind the save: consumed at the end, not yet at the save
        assert _summary_fields(r.ck) == (1 + PRE_OBSERVES + PRE, 0)
        assert _summary_fields(r.end_ck[1]) == (1 + PRE_OBSERVES + PRE + POST, 1)


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_a_checkpoint_survives_a_file(torch_mod, tmp, name):
    r = _continuation(name, tmp)
    assert r.from_file.blob == r.ck.blob and torch_mod.equal(r.from_file.block, r.ck.block)
    _same_checkpoint(r.ck, r.from_file, "file")
    assert bytes(r.from_file.cfg) == bytes(r.ck.cfg)
    assert r.from_file.obs.dtype == r.ck.obs.dtype


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_restore_into_the_same_handle_after_it_has_run_on(torch_mod, tmp, name):
    r = _continuation(name, tmp)
    _same_steps(r.first, r.third, "same handle")
    _same_state(r.end[0], r.end[2], "same handle")
    _same_checkpoint(r.end_ck[0], r.end_ck[2], "same handle")


def test_restore_refuses_other_outputs(torch_mod, tmp):
    from antsrl_amd import _lib
    r = _continuation("a_base", tmp)
    with pytest.raises(ValueError, match="obs"):
        _make("g_bf16").restore(r.ck)  # the same AntsCfg, bfloat16 observations
    with pytest.raises(ValueError):
        _make("f_one_env").restore(r.ck)
    other = _make("a_base", max_time=77)  # equal shapes, another AntsCfg: the library's refusal, the field named
    with pytest.raises(_lib.AntsrlError, match="max_time"):
        other.restore(r.ck)


def test_a_handle_between_two_update_phases_is_refused(torch_mod, tmp):
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    r = _continuation("a_base", tmp)
    env = _make("a_base")
    env.observe()
    env.update_phase(cm.PHASE_WALLS)
    for call in (env.checkpoint, lambda: env.restore(r.ck), lambda: env.fork([1], [0])):
        with pytest.raises(_lib.AntsrlError, match="Environment.update is in progress"):
            call()
    for phase in (cm.PHASE_ROCKS_PHEROMONE, cm.PHASE_ANTS, cm.PHASE_ANTHILL):
        env.update_phase(phase)
    env.fork([1], [0])
    torch_mod.cuda.synchronize()


# ---- fork -----------------------------------------------------------------------------------------------------------------
SRC, DST = [1, 1, 3], [0, 4, 2]


def _aged(name, wall_density, jitter_seed=None):
    """An env 20 steps into its episode (the environments have grown apart), flushed."""
    env = _make(name, wall_density=wall_density)
    env.observe()
    rot, ph = _actions(env.cfg, 20, seed=5)
    _run(env, rot, ph)
    env.flush()
    return env


@pytest.mark.parametrize("walls", [False, True], ids=["no_walls_library_jitter", "walls_explicit_jitter"])
def test_fork_copies_the_rows_and_the_branches_repeat_their_sources(torch_mod, walls):
    torch = torch_mod
    env = _aged("a_base", 0.08 if walls else 0.0)
    cfg = env.cfg
    before, out_before = _read_all(env), _outputs(env)
    env.fork(SRC, DST)
    after, out_after = _read_all(env), _outputs(env)
    others = [e for e in range(cfg.n_envs) if e not in DST]
    for w in before:  # right after the fork: each dst's rows are its src's, every other environment's are untouched
        assert torch.equal(after[w][DST], before[w][SRC]), "selector %d: a dst row is not its src's" % w
        assert torch.equal(after[w][others], before[w][others]), "selector %d: another environment's row changed" % w
    for k, u, v in zip(("obs", "agent_state", "reward", "done"), out_before, out_after):
        assert torch.equal(v[DST], u[SRC]) and torch.equal(v[others], u[others]), k
    assert not torch.equal(before[0][0], before[0][1])  # (the environments did differ)
    rot, ph = _actions(cfg, 30, seed=23)
    rot[:, DST], ph[:, DST] = rot[:, SRC], ph[:, SRC]  # each dst gets its src's actions
    jitter = None
    if walls:  # explicit wall jitter, the src's rows for the dst
        jitter = torch.as_tensor(np.random.default_rng(7).random((30, cfg.n_envs, cfg.n_ants))).cuda()
        jitter[:, DST] = jitter[:, SRC]
    for t, (obs, ast, rw, dn) in enumerate(_run(env, rot, ph, jitter)):
        for k, v in (("obs", obs), ("agent_state", ast), ("reward", rw), ("done", dn)):
            assert torch.equal(v[DST], v[SRC]), "%s of a dst differs from its src's at step %d" % (k, t)
    end = _read_all(env)
    for w in end:
        assert torch.equal(end[w][DST], end[w][SRC]), "selector %d at the end" % w
    assert not torch.equal(end[0][1], end[0][3])


def _ws_entries(env, split):
    from antsrl_amd import _lib
    n = C.c_int32()
    assert env.lib.antsrl_workspace_map(C.byref(env.cfg), split, None, 0, C.byref(n)) == 0
    arr = (_lib.AntsWsArray * n.value)()
    assert env.lib.antsrl_workspace_map(C.byref(env.cfg), split, arr, n.value, C.byref(n)) == 0
    return [(a.name.decode(), a.block, int(a.offset), int(a.bytes)) for a in arr]


@pytest.mark.parametrize("name", ["a_base", "c_diffuse3x3", "e_single_kernel"])
def test_fork_writes_the_dst_rows_and_no_other_byte_of_the_workspace(torch_mod, name):
    """The whole workspace, both blocks with their alignment slack, the padding between the arrays and pol_pack: after the
    fork it is what it was, but for each dst's row of each array, which is its src's — so the byte in front of and behind
    every forked row is unchanged.  (The blocks were filled with 0xA5 before the reset.)"""
    torch = torch_mod
    env = _make(name, fill=0xA5)
    env.observe()
    rot, ph = _actions(env.cfg, 12, seed=5)
    _run(env, rot, ph)
    env.flush()
    torch.cuda.synchronize()
    blocks = {0: (env._state, env._state_ptr - env._state.data_ptr()), 1: (env._ws, env._ws_ptr - env._ws.data_ptr())}
    before = {b: t.clone() for b, (t, _) in blocks.items()}
    expected = {b: t.clone() for b, t in before.items()}
    E = env.cfg.n_envs
    for aname, block, offset, nbytes in _ws_entries(env, 1):
        if aname == "pol_pack":
            continue
        t, base = blocks[block]
        rows = t[base + offset: base + offset + nbytes].view(E, nbytes // E)
        expected[block][base + offset: base + offset + nbytes].view(E, nbytes // E)[DST] = rows[SRC]
    env.fork(SRC, DST)
    torch.cuda.synchronize()
    for b, (t, _) in blocks.items():
        diff = (t != expected[b]).nonzero().view(-1)
        assert diff.numel() == 0, "block %d: %d bytes differ, the first at %d" % (b, diff.numel(), int(diff[0]))
        assert not torch.equal(t, before[b])  # (each block holds forked rows)


@pytest.mark.parametrize("name", ["a_base", "c_diffuse3x3", "f_one_env"])
def test_save_writes_the_arrays_and_no_other_byte_of_the_block(torch_mod, name):
    """A block with 256 bytes of padding on either side, filled with 0x5C: antsrl_checkpoint_save leaves the padding and
    the bytes between an array's end and the next array's start as they were, and antsrl_checkpoint_load reads the block
    without changing it."""
    torch = torch_mod
    from antsrl_amd import _lib
    from antsrl_amd.checkpoint import checkpoint_map
    env = _make(name)
    env.observe()
    rot, ph = _actions(env.cfg, 5, seed=5)
    _run(env, rot, ph)
    entries, dev, host = checkpoint_map(env.cfg)
    E = env.cfg.n_envs
    buf = torch.full((dev + 512,), 0x5C, dtype=torch.uint8, device=env.device)
    assert buf.data_ptr() % 256 == 0
    blob = C.create_string_buffer(host)
    _lib.check(env.lib.antsrl_checkpoint_save(env._h, C.c_void_p(buf.data_ptr() + 256), blob, env._stream()))
    torch.cuda.synchronize()
    written = torch.zeros((dev + 512,), dtype=torch.bool, device=env.device)
    for _, off, bpe in entries:
        written[256 + off: 256 + off + bpe * E] = True
    assert int((~written).sum()) >= 512 + 200  # (there are gaps: most arrays are no multiple of 256 bytes)
    assert bool((buf[~written] == 0x5C).all()), "a byte outside the arrays was written"
    ck = env.checkpoint()
    assert torch.equal(buf[256:256 + dev][written[256:256 + dev]], ck.block[written[256:256 + dev]])
    assert blob.raw == ck.blob
    snapshot = buf.clone()
    _lib.check(env.lib.antsrl_checkpoint_load(env._h, C.c_void_p(buf.data_ptr() + 256), blob, env._stream()))
    torch.cuda.synchronize()
    assert torch.equal(buf, snapshot)
    # a block inside the workspace is refused before anything is enqueued
    rc = env.lib.antsrl_checkpoint_save(env._h, C.c_void_p(env._ws_ptr + 256), blob, env._stream())
    assert rc == -1 and b"overlaps the handle's workspace" in env.lib.antsrl_last_error()


# ---- the loop -------------------------------------------------------------------------------------------------------------
def _agent(kind):
    from antsrl_amd import agent as ag
    kw = dict(epsilon=0.3, replay_size=512, min_replay=64, minibatch=32, learning_rate=1e-3, seed=7)
    return {"collect": ag.CollectAgent, "explore": ag.ExploreAgent, "rework": ag.ReworkAgent, "memory": ag.MemoryAgent}[kind](**kw)


def _loop_env(seed):
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    cfg = cm.make_cfg(2, 16, 32, 32, deposit_strength=256.0, max_time=30)
    env = BatchedAntsEnv(cfg)
    env.reset(synth_init(cfg, seed=seed, n_food_discs=4, food_rmin=2, food_rmax=4))
    return env


def _loop(agent, env, steps):
    losses, rewards = [], []
    for _ in range(steps):
        loss = agent.rollout_step(env)
        losses.append(float(loss))
        rewards.append(env.reward.clone())
    return losses, rewards


def _same_dict(a, b, what):
    import torch
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], dict):
            _same_dict(a[k], b[k], "%s.%s" % (what, k))
        elif isinstance(a[k], list):
            _same_dict(dict(enumerate(a[k])), dict(enumerate(b[k])), "%s.%s" % (what, k))
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), "%s.%s differs" % (what, k)
        else:
            assert a[k] == b[k], "%s.%s: %r != %r" % (what, k, a[k], b[k])


@pytest.mark.parametrize("kind", ["collect", "explore", "rework", "memory"])
def test_the_loop_continues_bit_for_bit(torch_mod, tmp, kind):
    torch = torch_mod
    from agent_harness import same_rings
    from antsrl_amd.checkpoint import EnvCheckpoint
    env, agent = _loop_env(5), _agent(kind)
    agent.setup(env)
    agent.initialize(env)
    env.observe()
    _loop(agent, env, 24)
    assert agent.trainer.step_count > 0 and agent.trainer.syncs == 0  # training has begun, the episode has not ended
    env.checkpoint().save("%s/%s_env.ckpt" % (tmp, kind))
    torch.save(agent.training_state(), "%s/%s_agent.pt" % (tmp, kind))
    losses, rewards = _loop(agent, env, 24)
    assert agent.trainer.syncs == 1 and any(l != 0 for l in losses)  # (done at step 30: the target's sync lies behind the save)

    env2, agent2 = _loop_env(23), _agent(kind)  # another episode, fresh weights
    agent2.setup(env2)
    env2.restore(EnvCheckpoint.load("%s/%s_env.ckpt" % (tmp, kind), env2.device))
    agent2.load_training_state(torch.load("%s/%s_agent.pt" % (tmp, kind), map_location=env2.device))
    losses2, rewards2 = _loop(agent2, env2, 24)

    assert losses == losses2, (losses, losses2)
    for t, (u, v) in enumerate(zip(rewards, rewards2)):
        assert torch.equal(u, v), "the rewards differ at step %d" % t
    t1, t2 = agent.trainer, agent2.trainer
    _same_dict(t1.state_dict(), t2.state_dict(), "state_dict")
    _same_dict(t1.target_state_dict(), t2.target_state_dict(), "target_state_dict")
    _same_dict(t1.adam_state(), t2.adam_state(), "adam_state")
    assert (t1.step_count, t1.target_update_counter, t1.syncs) == (t2.step_count, t2.target_update_counter, t2.syncs)
    same_rings(agent.replay_memory, agent2.replay_memory,
               ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones"))
    assert (agent.step_counter, agent.epsilon) == (agent2.step_counter, agent2.epsilon)
    _same_dict(agent.training_state(), agent2.training_state(), "training_state")
