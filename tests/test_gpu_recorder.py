"""EpisodeRecorder (antsrl_amd/recorder.py; include/antsrl.h, "The episode recorder") against the path it replaces, bit for
bit: twelve random-action step_updates with record() after each on one environment, snapshot_batched and read_state after
each of the same steps on a twin, and a third environment that never records.

Cases (CASES; not the full product): the shapes (1, 1, 64, 64), (3, 50, 64, 64), (4, 65, 48, 80), (2, 257, 64, 64) and 9
environments with 8 selected; the step paths ACT_CELL_META, the default and ACT_SINGLE_KERNEL (k_act's bit maps: the
default resolves to the cell-meta path for these channel lists); an explicit 3 x 3 diffusion (separate pheromone buffers,
`cur` flips every update; {food, META} records tiled 4 x 4 and row-major); REWARD_FOOD (no heatmap section); 3 rocks; 1 and
3 pheromone channels; the selections [0], [E - 1], [2, 0] and 8 of 9.  make_cfg sets no lower bound on a grid; 12 cells
is the smallest side the suite steps anywhere (tests/test_gpu_fuzz.py), so the small non-square grids are 12 x 13 (156
cells: the smallest such grid that is no multiple of 16) and 13 x 15 (195 cells: no multiple of 4 either, the last packed
word of every grid section is a tail).  deposit_strength = 256 everywhere, so the uint8 pheromone is not all 0 or 1."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import recorder_ref as R

pytestmark = pytest.mark.gpu

STEPS, GUARD, FILL = 12, 4096, 0xA5


def _cases():
    from antsrl_amd import config as cm
    meta, single = dict(act_path=cm.ACT_CELL_META), dict(act_path=cm.ACT_SINGLE_KERNEL)
    diffuse = dict(filt=cm.diffuse_filter(0.05, 0.001))
    return {  # name: (E, N, W, H, make_cfg keywords, selection)
        "one-ant-meta": (1, 1, 64, 64, meta, [0]),
        "one-ant-default": (1, 1, 64, 64, {}, [0]),
        "one-ant-k_act": (1, 1, 64, 64, single, [0]),
        "3x50-default-last": (3, 50, 64, 64, {}, [2]),
        "3x50-k_act-2-0": (3, 50, 64, 64, single, [2, 0]),
        "4x65-48x80-meta-2-0": (4, 65, 48, 80, meta, [2, 0]),
        "4x65-48x80-k_act-last": (4, 65, 48, 80, single, [3]),
        "2x257-meta": (2, 257, 64, 64, meta, [1]),
        "2x257-default-both": (2, 257, 64, 64, {}, [1, 0]),
        "8-of-9": (9, 50, 64, 64, {}, [8, 0, 1, 2, 3, 5, 6, 7]),
        "diffusion-3x3": (3, 50, 64, 64, diffuse, [2, 0]),
        "diffusion-3x3-meta-13x15": (2, 5, 13, 15, dict(meta, **diffuse), [1]),
        "diffusion-3x3-k_act": (3, 50, 64, 64, dict(single, **diffuse), [0]),
        "reward-food": (3, 50, 64, 64, dict(reward_kind=cm.REWARD_FOOD), [0]),
        "reward-all": (3, 50, 64, 64, dict(reward_kind=cm.REWARD_ALL), [1]),
        "rocks-3": (3, 50, 64, 64, dict(n_rocks=3), [2, 0]),
        "rocks-3-k_act": (4, 65, 48, 80, dict(single, n_rocks=3), [0]),
        "one-pheromone": (3, 50, 64, 64, dict(n_phero=1), [2, 0]),
        "three-pheromones": (3, 50, 64, 64, dict(n_phero=3), [0]),
        "12x13": (2, 7, 12, 13, {}, [1, 0]),
        "13x15": (2, 5, 13, 15, {}, [0]),
        "13x15-k_act": (2, 5, 13, 15, single, [1]),
    }


NAMES = ["one-ant-meta", "one-ant-default", "one-ant-k_act", "3x50-default-last", "3x50-k_act-2-0", "4x65-48x80-meta-2-0",
         "4x65-48x80-k_act-last", "2x257-meta", "2x257-default-both", "8-of-9", "diffusion-3x3", "diffusion-3x3-meta-13x15",
         "diffusion-3x3-k_act", "reward-food", "reward-all", "rocks-3", "rocks-3-k_act", "one-pheromone", "three-pheromones",
         "12x13", "13x15", "13x15-k_act"]


def make(E, N, W, H, kw, seed=5):
    """A small environment in the style of agent_harness.make_env."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    cfg = cm.make_cfg(E, N, W, H, deposit_strength=256.0, max_time=2000, **kw)
    env = BatchedAntsEnv(cfg)
    small = min(W, H) < 32
    env.reset(synth_init(cfg, seed=seed, n_food_discs=6, food_rmin=1 if small else 3, food_rmax=3 if small else 6))
    return env


def guarded_recorder(env, sel, max_frames=STEPS, **kw):
    """A recorder over a block with GUARD sentinel bytes in front and behind."""
    import torch
    from antsrl_amd.recorder import EpisodeRecorder
    probe = EpisodeRecorder(env, env_indices=sel, max_frames=max_frames, **kw)
    buf = torch.full((GUARD + probe.bytes + GUARD,), FILL, dtype=torch.uint8, device=env.device)
    return EpisodeRecorder(env, env_indices=sel, max_frames=max_frames, block=buf[GUARD: GUARD + probe.bytes], **kw), buf


def actions(cfg, device, seed=11):
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    rot = torch.randint(-1, 2, (STEPS, cfg.n_envs, cfg.n_ants), generator=g, device=device, dtype=torch.int8)
    ph = torch.randint(0, 3, (STEPS, cfg.n_envs, cfg.n_ants), generator=g, device=device, dtype=torch.int8) if cfg.n_phero == 2 else [None] * STEPS
    return rot, ph


@functools.lru_cache(maxsize=None)
def run(name):
    """The three runs of a case, once: everything the tests below compare, on the host."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd import snapshot
    E, N, W, H, kw, sel = _cases()[name]
    rec_env, twin, plain = make(E, N, W, H, kw), make(E, N, W, H, kw), make(E, N, W, H, kw)
    cfg = rec_env.cfg
    if cfg.n_phero != 2:  # no pheromone actions (ants.py:89-96 takes two channels): every ant deposits on every channel
        for env in (rec_env, twin, plain):
            env.set_activation(torch.full((E, N, cfg.n_phero), 10.0, device=env.device))
    rot, ph = actions(cfg, rec_env.device)
    rec, buf = guarded_recorder(rec_env, sel)
    # ---- recorded: nothing is read back inside the loop
    rec.begin()
    outs, blocks = [], []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(STEPS):
            rec_env.step_update(rot[t], ph[t])
            rec.record()
            outs.append((rec_env.reward.clone(), rec_env.obs.clone(), rec_env.done.clone()))
            blocks.append(rec.block.clone())
    finally:
        torch.cuda.set_sync_debug_mode(0)
    n_frames = rec.n_frames
    frames, states = rec.frames(), rec.snapshots()
    # ---- one frame too many: raises on the host, and the C entry refuses the slot; the block stays as it is
    before = rec.block.clone()
    from antsrl_amd import _lib
    with pytest.raises(_lib.AntsrlError, match="max_frames"):
        rec.record()
    rc = rec._lib.antsrl_recorder_frame(*rec._args(), STEPS, rec_env._stream())
    overrun = SimpleNamespace(rc=rc, message=rec._lib.antsrl_last_error(), unchanged=torch.equal(rec.block, before), n_frames=rec.n_frames)
    # ---- the twin: the path the recorder replaces, after each of the same steps
    which = dict(timestep=cm.S_TIMESTEP, anthill_food=cm.S_ANTHILL_FOOD, ants_xyt=cm.S_ANTS_XYT, holding=cm.S_HOLDING,
                 mandibles=cm.S_MANDIBLES, reward_state=cm.S_REWARD_STATE, phero=cm.S_PHERO, food=cm.S_FOOD,
                 explored=cm.S_EXPLORED, walls=cm.S_WALLS, anthill_xyr=cm.S_ANTHILL_XYR)
    if cfg.n_rocks:
        which.update(rock_centers=cm.S_ROCK_CENTERS, rock_rw=cm.S_ROCK_RW)
    twin_states, reads = [], []
    for t in range(STEPS):
        twin.step_update(rot[t], ph[t])
        twin_states.extend(snapshot.snapshot_batched(twin, sel))
        reads.append({k: twin.read_state(w).cpu().numpy()[sel] for k, w in which.items()})
    # ---- the third environment never records
    plain_outs = []
    for t in range(STEPS):
        plain.step_update(rot[t], ph[t])
        plain_outs.append((plain.reward.clone(), plain.obs.clone(), plain.done.clone()))
    same_outs = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                    for x, y in zip(outs, plain_outs) for a, b in zip(x, y))
    finals = {k: (rec_env.read_state(w).cpu().numpy(), plain.read_state(w).cpu().numpy()) for k, w in (("xyt", cm.S_ANTS_XYT), ("phero", cm.S_PHERO))}
    return SimpleNamespace(cfg=cfg, sel=sel, rec=rec, n_frames=n_frames, frames=frames, states=states, twin_states=twin_states,
                           reads=reads, same_outs=same_outs, finals=finals, overrun=overrun, buf=buf.cpu().numpy(),
                           blocks=[b.cpu().numpy() for b in blocks], before=before.cpu().numpy())


@pytest.mark.parametrize("name", NAMES)
def test_snapshots_pickle_to_the_bytes_of_snapshot_batched(name):
    from antsrl_amd import snapshot
    r = run(name)
    assert r.n_frames == STEPS and len(r.states) == len(r.twin_states) == STEPS * len(r.sel)
    assert snapshot.dumps(r.states) == snapshot.dumps(r.twin_states)
    keeps_map = r.cfg.reward_kind in (1, 3)
    assert (r.states[0].objects[-1].heatmap is None) == (not keeps_map)
    assert ("explored" in r.frames) == keeps_map  # (without a map the section is absent, not zero)


@pytest.mark.parametrize("name", NAMES)
def test_frames_equal_read_state_field_by_field(name):
    r = run(name)
    c, S = r.cfg, len(r.sel)
    f = r.frames
    assert f["phero"].shape == (STEPS, S, c.n_phero, c.w, c.h) and f["ants_xyt"].shape == (STEPS, S, c.n_ants, 3)
    seen_above_one = False
    for t, rd in enumerate(r.reads):
        for k, want in rd.items():
            if k == "explored" and "explored" not in f:
                continue
            got = f[k] if k in ("walls", "anthill_xyr", "rock_rw") else f[k][t]
            if k in ("phero", "food"):
                assert want.max() < 256 and want.min() >= 0  # where numpy's astype and the header's cast are one rule
                assert np.array_equal(want.astype(np.uint8), R.cast_u8(want))
                want = R.cast_u8(want)
                seen_above_one |= k == "phero" and bool((want > 1).any())
            assert got.dtype == want.dtype and got.shape == want.shape, (k, t, got.dtype, want.dtype, got.shape, want.shape)
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (k, t)  # every bit
    assert seen_above_one or c.n_ants == 1, "the recorded pheromone never exceeds 1"  # (a lone ant may never deposit in 12 steps)
    # the product's decoding against the layout restated from the header's text, on the block's own bytes
    block = r.buf[GUARD: GUARD + r.rec.bytes]
    ref = R.decode(block, S, c.n_ants, c.w, c.h, c.n_phero, c.n_rocks, "explored" in f, STEPS)
    assert sorted(ref) == sorted(f)
    for k in ref:
        assert ref[k].dtype == f[k].dtype and np.array_equal(ref[k].view(np.uint8), f[k].view(np.uint8)), k
    st, fr, tot = R.sizes(S, c.n_ants, c.w, c.h, c.n_phero, c.n_rocks, "explored" in f, STEPS)
    assert (st, fr, tot) == (r.rec.static_bytes, r.rec.frame_bytes, r.rec.bytes)


@pytest.mark.parametrize("name", NAMES)
def test_recording_does_not_perturb_the_run(name):
    r = run(name)
    assert r.same_outs, "reward, obs or done differ from the environment that never records"
    for k, (a, b) in r.finals.items():
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


@pytest.mark.parametrize("name", NAMES)
def test_overrun_protection(name):
    r = run(name)
    n = r.rec.bytes
    assert (r.buf[:GUARD] == FILL).all() and (r.buf[GUARD + n:] == FILL).all() and len(r.buf) == n + 2 * GUARD
    # a frame too many
    assert r.overrun.rc == -1 and b"frame %d" % STEPS in r.overrun.message and r.overrun.unchanged and r.overrun.n_frames == STEPS
    assert np.array_equal(r.before, r.blocks[-1])
    # frame f, and everything in front of it, is unchanged by writing frame f + 1
    st, fr = r.rec.static_bytes, r.rec.frame_bytes
    for t in range(STEPS - 1):
        assert np.array_equal(r.blocks[t + 1][: st + (t + 1) * fr], r.blocks[t][: st + (t + 1) * fr]), t
        assert (r.blocks[t][st + (t + 1) * fr:] == FILL).all(), t  # and nothing behind frame t is written early
    # every byte of the used block is written (sections and their zero padding): none keeps the fill pattern by accident
    fresh = r.blocks[-1]
    off = {(w, wh, nm): o for w, wh, nm, o in R.section_offsets(len(r.sel), r.cfg.n_ants, r.cfg.w, r.cfg.h, r.cfg.n_phero, r.cfg.n_rocks,
                                                              "explored" in r.frames, STEPS)}
    g, gp = r.cfg.w * r.cfg.h, R.a16(r.cfg.w * r.cfg.h)
    for (w, wh, nm), o in off.items():
        if nm in ("walls", "food", "explored") or nm.startswith("phero"):
            assert (fresh[o + g: o + gp] == 0).all(), (w, wh, nm)


@pytest.mark.parametrize("kw", [{}, dict(act_path=2)], ids=["default", "k_act"])
def test_a_second_begin_takes_the_new_map(kw):
    """begin() again after env.generate with another seed: the new walls and anthill, and frames from zero."""
    import torch
    from antsrl_amd import config as cm
    env = make(3, 50, 64, 64, kw)
    gen = cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)
    rec, buf = guarded_recorder(env, [2, 0], max_frames=4)
    rot, ph = actions(env.cfg, env.device)
    seen = []
    for seed in (21, 22):
        env.generate(gen, seed)
        env.observe()
        rec.begin()
        assert rec.n_frames == 0
        for t in range(2):
            env.step_update(rot[t], ph[t])
            rec.record()
        f = rec.frames()
        assert rec.n_frames == 2 and f["timestep"].tolist() == [[2, 2], [3, 3]]
        walls, xyr = env.read_state(cm.S_WALLS).cpu().numpy()[[2, 0]], env.read_state(cm.S_ANTHILL_XYR).cpu().numpy()[[2, 0]]
        assert np.array_equal(f["walls"], walls) and np.array_equal(f["anthill_xyr"], xyr)
        assert np.array_equal(f["ants_xyt"][1].view(np.uint8), env.read_state(cm.S_ANTS_XYT).cpu().numpy()[[2, 0]].view(np.uint8))
        seen.append((walls, xyr))
    assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[0][1], seen[1][1])
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + rec.bytes:] == FILL).all()


def test_refused_while_an_update_is_in_progress_and_on_a_selection_outside_the_batch():
    """The two refusals that need a handle that has been reset: an Environment.update in progress (antsrl_update_phase
    outstanding), for begin and for record, the block untouched; and the index checks against a live batch."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.recorder import EpisodeRecorder
    env = make(3, 50, 64, 64, {})
    rec, buf = guarded_recorder(env, [1], max_frames=3)
    rot, ph = actions(env.cfg, env.device)
    rec.begin()
    env.step(rot[0], ph[0])
    env.update_phase(cm.PHASE_WALLS)
    before = buf.clone()
    for call in (rec.record, rec.begin):
        with pytest.raises(_lib.AntsrlError, match="in progress"):
            call()
    assert torch.equal(buf, before) and rec.n_frames == 0
    for phase in (cm.PHASE_ROCKS_PHEROMONE, cm.PHASE_ANTS, cm.PHASE_ANTHILL):
        env.update_phase(phase)
    rec.record()
    assert rec.n_frames == 1 and rec.frames()["timestep"].tolist() == [[2]]
    spare = torch.full((1 << 20,), FILL, dtype=torch.uint8, device=env.device)
    for bad, word in (([3], "n_envs = 3"), ([0, 0], "repeats"), ([], "n_sel"), (list(range(3)) * 3, "n_sel")):
        with pytest.raises(_lib.AntsrlError, match=word):
            r2 = EpisodeRecorder(env, env_indices=bad, max_frames=3, block=spare)
            r2.begin()
    assert bool((spare == FILL).all())
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + rec.bytes:] == FILL).all()
