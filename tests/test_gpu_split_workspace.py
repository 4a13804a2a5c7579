"""A handle over two workspace blocks (antsrl_create2: cell records apart from everything else) against a handle over one
block (antsrl_create), same seed: every output and every state array read back must be equal bit for bit.

The record block is allocated separately from the state block and lies BELOW it in memory, so code that assumed "the records
follow the per-ant arrays" would read or write the wrong block; both blocks sit inside guard bands whose pattern must
survive.  Shapes are the smallest that cross the seams: E = 3, N = 40 (no multiple of the perception run of 8 or of the
32-ant tile), a 16 x 12 grid (a 7 x 7 patch wraps on both axes), one rock; a radius-1 filter at E = 2 on 16 x 16 for the
separate pheromone buffers and {food, META} records; and the single-kernel path on the first shape.  The sequence: reset,
steps with a deferred update, a state read in between (which enqueues the pending update), a step and an update on their
own, a snapshot restored through reset, a device-generated episode."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = 0xA5


def _diffuse3():
    f3 = np.ones((3, 3)) * 0.02
    f3[1, 1] = 1 - 8 * 0.02
    return f3 * (1 - 0.001)


def _cases():
    from antsrl_amd import config as cm
    return {
        "interleaved": lambda: cm.make_cfg(3, 40, 16, 12, n_rocks=1, deposit_strength=256.0),
        "radius1": lambda: cm.make_cfg(2, 40, 16, 16, deposit_strength=256.0, filt=_diffuse3()),
        "single_kernel": lambda: cm.make_cfg(3, 40, 16, 12, n_rocks=1, deposit_strength=256.0, act_path=cm.ACT_SINGLE_KERNEL),
    }


def _guarded_blocks(env):
    """The record block and the state block as the interiors of two separate allocations, records at the lower address, each
    with GUARD bytes of PATTERN on either side."""
    import torch
    n = max(env.record_bytes, env.state_bytes) + 2 * GUARD + 512
    a = torch.full((n,), PATTERN, dtype=torch.uint8, device=env.device)  # (the record block first)
    b = torch.full((n,), PATTERN, dtype=torch.uint8, device=env.device)
    lo, hi = (a, b) if a.data_ptr() < b.data_ptr() else (b, a)

    def interior(buf, nbytes):
        start = GUARD + (-(buf.data_ptr() + GUARD)) % 256
        return buf[start:start + nbytes], (buf, start, start + nbytes)
    rec, rec_guard = interior(lo, env.record_bytes)
    st, st_guard = interior(hi, env.state_bytes)
    assert rec.data_ptr() + env.record_bytes <= st.data_ptr()
    return rec, st, (rec_guard, st_guard)


def _selectors(cfg):
    from antsrl_amd import config as cm
    sel = [cm.S_ANTS_XYT, cm.S_PREV_XY, cm.S_HOLDING, cm.S_MANDIBLES, cm.S_ACTIVATION, cm.S_PHERO, cm.S_FOOD, cm.S_EXPLORED,
           cm.S_ANTHILL_FOOD, cm.S_TIMESTEP, cm.S_REWARD_STATE, cm.S_WALLS, cm.S_ANTHILL_AREA, cm.S_SEED, cm.S_ANTHILL_XYR,
           cm.S_PHERO_C0, cm.S_PHERO_C1]
    if cfg.n_rocks:
        sel += [cm.S_ROCK_CENTERS, cm.S_ROCK_RW]
    return sel


@pytest.mark.parametrize("name", ["interleaved", "radius1", "single_kernel"])
def test_split_handle_equals_single_block_handle(name):
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    cfg = _cases()[name]()
    one = BatchedAntsEnv(cfg, split_workspace=False)
    two = BatchedAntsEnv(cfg)
    assert one._state is None and two.state_bytes + two.record_bytes == one.workspace_bytes
    rec, st, guards = _guarded_blocks(two)
    two._make_handle(rec, st)
    assert two._ws_ptr == rec.data_ptr() and two._state_ptr == st.data_ptr() and two._ws_ptr < two._state_ptr
    if name == "interleaved":
        assert two.query(cm.Q_INTERLEAVED) == 1 and two.query(cm.Q_CELL_META) == 1 and two.query(cm.Q_DEFERRED_UPDATE) == 1
    elif name == "radius1":
        assert two.query(cm.Q_INTERLEAVED) == 0 and two.query(cm.Q_SCALED_UNITS) == 0
    else:
        assert two.query(cm.Q_CELL_META) == 0
    envs = (one, two)
    steps_done = 0

    def same_outputs(outs):
        for x, y in zip(*outs):
            assert torch.equal(x, y)

    def same_state(what):
        for which in _selectors(cfg):
            a, b = one.read_state(which), two.read_state(which)
            assert torch.equal(a, b), "%s: state array %d differs" % (what, which)

    init = synth_init(cfg, seed=11, n_food_discs=3, food_rmin=1, food_rmax=3)
    rot, ph = random_actions(cfg, 8, seed=5)
    for env in envs:
        env.reset(init)
    same_outputs([env.observe() for env in envs])
    for t in range(2):  # (each leaves an update deferred where the path defers)
        same_outputs([env.step_update(rot[t], ph[t], None) for env in envs])
        steps_done += 1
    same_state("after two steps, an update pending")  # (the first read enqueues it)
    same_outputs([env.step(rot[2], ph[2]) for env in envs])
    for env in envs:
        env.update()
    steps_done += 1
    same_outputs([env.step_update(rot[3], ph[3], None) for env in envs])
    steps_done += 1
    for env in envs:
        env.flush()
    same_state("after a step and an update on their own")

    # snapshot (the arrays antsrl_reset takes, read back), one more step, then the snapshot restored through reset
    def snapshot(env):
        rd = lambda w: env.read_state(w).cpu().numpy()  # noqa: E731
        s = dict(ants_xyt=rd(cm.S_ANTS_XYT), seed=rd(cm.S_SEED).astype(np.float64), walls=rd(cm.S_WALLS), food=rd(cm.S_FOOD),
                 anthill_xyr=rd(cm.S_ANTHILL_XYR), phero=rd(cm.S_PHERO))
        if cfg.n_rocks:
            s["rocks"] = np.concatenate([rd(cm.S_ROCK_CENTERS), rd(cm.S_ROCK_RW)], axis=-1)
        return s
    snaps = [snapshot(env) for env in envs]
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k], snaps[1][k]), k
    same_outputs([env.step_update(rot[4], ph[4], None) for env in envs])
    steps_done += 1
    for env, s in zip(envs, snaps):
        env.reset(s)
    same_outputs([env.observe() for env in envs])
    same_outputs([env.step_update(rot[4], ph[4], None) for env in envs])
    steps_done += 1
    same_state("after the restored snapshot")

    # a device-generated episode over the same blocks
    for env in envs:
        env.generate(cm.make_gen(n_food_discs=3, food_rmin=1, food_rmax=3), episode_seed=77)
    for t in (5, 6):
        same_outputs([env.step_update(rot[t], ph[t], None) for env in envs])
        steps_done += 1
    same_state("after generate")
    assert steps_done >= 6
    torch.cuda.synchronize()
    for buf, lo, hi in guards:
        assert bool((buf[:lo] == PATTERN).all()) and bool((buf[hi:] == PATTERN).all()), "a kernel wrote outside its block"
