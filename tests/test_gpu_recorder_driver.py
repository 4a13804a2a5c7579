"""train_episodes(..., snapshot_on_device=True) (antsrl_amd/driver.py) against the same call without it: ReworkAgent, 3
episodes of 8 steps, 3 environments of 64 ants, snapshot_every = 2 (episodes 0 and 1 are visualised).  The pickled states
are equal byte for byte, the statistics, the epsilons and the trained weights in every bit: recording on the device
perturbs nothing.  The steps of the recorded episodes run under a sync debug mode that makes any read-back an error."""
import numpy as np
import pytest

import monitor_ref as R
from agent_harness import make_env

pytestmark = pytest.mark.gpu

E, N, STEPS, EPISODES, SEED = 3, 64, 8, 3, 21


def the_gen():
    from antsrl_amd import config as cm
    return cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)


def make_agent():
    """Training starts inside the first episode: 192 rows per step against min_replay = 300."""
    from antsrl_amd.agent import ReworkAgent
    return ReworkAgent(epsilon=0.5, learning_rate=1e-3, min_replay=300, replay_size=3000, minibatch=64, seed=7)


def weights(agent):
    t = agent.trainer
    return {k: getattr(t, k) for k in ("model", "target", "heads", "target_l3") if hasattr(t, k)}


def quiet_steps(agent):
    """agent.rollout_step with every host read an error from the call's entry until the NEXT rollout_step begins or the
    episode's frames are read (recorder.frames lifts it): the monitor's step and recorder.record() fall in between."""
    import torch
    from antsrl_amd.recorder import EpisodeRecorder
    fused, read = agent.rollout_step, EpisodeRecorder.frames
    calls = dict(steps=0, reads=0)

    def step(env, training=True):
        torch.cuda.set_sync_debug_mode("error")
        calls["steps"] += 1
        return fused(env, training)

    def frames(self):
        torch.cuda.set_sync_debug_mode(0)
        calls["reads"] += 1
        return read(self)
    agent.rollout_step = step
    return frames, calls


def test_the_driver_with_the_recorder_equals_the_driver_with_snapshot_batched(monkeypatch):
    import torch
    from antsrl_amd import snapshot
    from antsrl_amd.driver import train_episodes
    from antsrl_amd.recorder import EpisodeRecorder
    env_a, a = make_env(E, N, STEPS), make_agent()
    a.setup(env_a)
    frames, calls = quiet_steps(a)
    monkeypatch.setattr(EpisodeRecorder, "frames", frames)
    torch.cuda.synchronize()
    try:
        # (two episodes, both visualised: every step of the run is a recorded episode's step)
        log = train_episodes(a, env_a, the_gen(), 2, STEPS, seed=SEED, snapshot_every=2, snapshot_on_device=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert calls == dict(steps=2 * STEPS, reads=2) and len(log["states"]) == 2 * STEPS
    monkeypatch.undo()
    # the comparison proper: three episodes each way, fresh agents
    env_a, env_b = make_env(E, N, STEPS), make_env(E, N, STEPS)
    a, b = make_agent(), make_agent()
    log_a = train_episodes(a, env_a, the_gen(), EPISODES, STEPS, seed=SEED, snapshot_every=2, snapshot_on_device=True)
    log_b = train_episodes(b, env_b, the_gen(), EPISODES, STEPS, seed=SEED, snapshot_every=2)
    assert len(log_a["states"]) == len(log_b["states"]) == 2 * STEPS
    assert snapshot.dumps(log_a["states"]) == snapshot.dumps(log_b["states"])
    for k in ("reports", "all_reward", "all_loss", "grand_total", "epsilons"):
        assert np.array_equal(R.bits(log_a[k]), R.bits(log_b[k])), k
    for k in ("report_episode", "report_step", "n_losses"):
        assert np.array_equal(log_a[k], log_b[k]), k
    assert a.epsilon == b.epsilon
    wa, wb = weights(a), weights(b)
    assert wa and a.trainer.step_count == b.trainer.step_count > 0
    for k in wa:
        assert torch.equal(wa[k].view(torch.int32), wb[k].view(torch.int32)), k


def test_other_environments_and_the_default_stay_as_they_were():
    """snapshot_envs picks the recorded environments (in order); without snapshot_on_device the keyword changes nothing."""
    from antsrl_amd import snapshot
    from antsrl_amd.driver import train_episodes
    logs = []
    for kw in (dict(snapshot_on_device=True, snapshot_envs=(2, 0)), dict(snapshot_envs=(2, 0)), {}):
        log = train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), 1, STEPS, seed=SEED, snapshot_every=2, **kw)
        logs.append(log["states"])
    assert len(logs[0]) == 2 * STEPS and len(logs[1]) == len(logs[2]) == STEPS
    assert snapshot.dumps(logs[1]) == snapshot.dumps(logs[2])               # unset: exactly what it does today (environment 0)
    assert snapshot.dumps(logs[0][1::2]) == snapshot.dumps(logs[2])         # environment 0 is the second of (2, 0)
    assert snapshot.dumps(logs[0][0::2]) != snapshot.dumps(logs[2])
