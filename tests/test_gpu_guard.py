"""Regression guard for the round-1 abort / run-to-run difference on the full c3 batch: the
observation copy-out must never store outside its own rows, for any ant count — in particular one that is not a
multiple of the per-wave run (odd tails, partly filled last workgroups) at the batch size where the fault showed.

The observation tensor is handed to the C-ABI as a slice of a larger buffer with GUARD BANDS in front of and
behind it; after stepping, the bands must be untouched, two handles fed the same inputs must agree bit for
bit, and every observation element must have been written (no canary left inside)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = -12345.5


def _guarded_obs(torch, env, band_elems=4096):
    """Re-points env.obs at the middle of a canary-filled buffer; returns (buffer, front band, back band)."""
    n = env.obs.numel()
    buf = torch.full((n + 2 * band_elems,), CANARY, dtype=env.obs.dtype, device=env.device)
    env.obs = buf[band_elems:band_elems + n].view(env.obs.shape)
    return buf, buf[:band_elems], buf[band_elems + n:]


@pytest.mark.parametrize("n_ants,envs,bf16", [(509, 1024, False), (511, 1024, True), (37, 64, False), (130, 40, False),
                                               (1023, 24, False)])
def test_copy_out_stays_inside_its_rows(n_ants, envs, bf16):
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    cfg = cm.make_cfg(envs, n_ants, 256, 256, n_rocks=8, deposit_strength=256.0)
    init = synth_init(cfg, seed=21)
    dt = torch.bfloat16 if bf16 else torch.float32
    a, b = BatchedAntsEnv(cfg, obs_dtype=dt), BatchedAntsEnv(cfg, obs_dtype=dt)
    bufs = [_guarded_obs(torch, e) for e in (a, b)]
    a.reset(init)
    b.reset(init)
    rot, ph = random_actions(cfg, 4, seed=5)
    for t in range(4):
        oa = a.step_update(rot[t], ph[t], None)
        ob = b.step_update(rot[t], ph[t], None)
        assert all(torch.equal(x, y) for x, y in zip(oa, ob)), "run-to-run difference at step %d" % t
        for _, front, back in bufs:
            assert bool((front == CANARY).all()) and bool((back == CANARY).all()), "store outside the observation tensor"
        assert not bool((oa[0] == CANARY).any()), "an observation element was never written"
    # the standalone observation (no action phases) goes through the same copy-out
    oa, ob = a.observe(), b.observe()
    assert torch.equal(oa[0], ob[0])
    for _, front, back in bufs:
        assert bool((front == CANARY).all()) and bool((back == CANARY).all())


def test_full_config2_batch_sampled_envs_vs_oracle():
    """The FULL BASELINE config-2 batch (256 envs x 256 ants, 256x256, 2 pheromone channels, no rocks): sampled
    environments follow the oracle for 8 steps."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    from oracle.oracle import Oracle
    from test_gpu_parity import check_obs
    E, N, steps, pick = 256, 256, 8, [0, 100, 255]
    cfg = cm.make_cfg(E, N, 256, 256, deposit_strength=256.0)
    cfg_s = cm.make_cfg(len(pick), N, 256, 256, deposit_strength=256.0)
    init = synth_init(cfg, seed=777)
    sub = {k: (None if v is None else np.ascontiguousarray(v[pick])) for k, v in init.items()}
    orc = Oracle(cfg_s, sub, n_threads=3)
    env = BatchedAntsEnv(cfg)
    env.reset(init)
    rot, ph = random_actions(cfg, steps, seed=31)
    rng = np.random.default_rng(3)
    for t in range(steps):
        jit = rng.random((E, N))
        obs, ast, rew, done = env.step_update(rot[t], ph[t], jit)
        o_obs, o_ast, o_rew, o_done = orc.step(rot[t][pick], ph[t][pick])
        orc.update(jit[pick])
        go = obs[pick].cpu().numpy()
        for j in range(len(pick)):
            check_obs(cfg_s, go[j], o_obs[j], "c2 step %d env %d" % (t, pick[j]))
        np.testing.assert_array_equal(rew[pick].cpu().numpy(), o_rew.astype(np.float32))
    np.testing.assert_array_equal(env.read_state(cm.S_FOOD).cpu().numpy()[pick], orc.food)
    np.testing.assert_array_equal(env.read_state(cm.S_EXPLORED).cpu().numpy()[pick], orc.explored)


def test_flush_makes_the_workspace_consistent():
    """antsrl_flush (include/antsrl.h, "WORKSPACE CONSISTENCY"): with a deferred update the workspace holds the pre-update
    state until the next step, a state read — or antsrl_flush.  After flush + stream sync nothing is owed any more: a later
    state read changes no byte of the workspace; without the flush it does (the read enqueues the update)."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    cfg = cm.make_cfg(6, 200, 64, 64, n_rocks=2, deposit_strength=256.0, act_path=cm.ACT_CELL_META)
    init = synth_init(cfg, seed=4, n_food_discs=5, food_rmin=2, food_rmax=5)
    rot, ph = random_actions(cfg, 3, seed=1)
    a, b = BatchedAntsEnv(cfg), BatchedAntsEnv(cfg)
    assert a.query(cm.Q_DEFERRED_UPDATE) == 1
    for env in (a, b):
        env.reset(init)
        for t in range(3):
            env.step_update(rot[t], ph[t], None)
    a.flush()
    a.flush()  # (idempotent: nothing pending the second time)
    torch.cuda.synchronize()
    ws_a, ws_b = a._ws.clone(), b._ws.clone()
    xa, xb = a.read_state(cm.S_ANTS_XYT), b.read_state(cm.S_ANTS_XYT)  # b: this read enqueues the deferred update
    torch.cuda.synchronize()
    assert torch.equal(xa, xb)
    assert torch.equal(a._ws, ws_a), "a state read after antsrl_flush must find nothing left to enqueue"
    assert not torch.equal(b._ws, ws_b), "without the flush the update was still owed (and the read ran it)"
    # ... and both handles go on identically
    oa, ob = a.step_update(rot[0], ph[0], None), b.step_update(rot[0], ph[0], None)
    for x, y in zip(oa, ob):
        assert torch.equal(x, y)
