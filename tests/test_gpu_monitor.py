"""EpisodeMonitor on the device against its restatement (tests/monitor_ref.py), bit for bit: the accumulate, both reports'
{total, min, max} in THE ORDER OF THE SUMS, the episode's row, the zeroed episode_reward and the carried running loss.

Seven steps with a report after the third and the sixth, end_episode, two more steps; the losses are 0-d device tensors and
host zeros in one sequence; the rewards are synthetic float32 of mixed signs, 1e-3 ... 1e3, with exact zeros and -0.0."""
import functools

import numpy as np
import pytest

import monitor_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1),      # a single ant
          (1, 50),     # main.py's own
          (3, 70),     # empty slots, N not a multiple of the wave
          (2, 256),    # exactly one ant per slot
          (2, 257),    # one slot with two ants
          (3, 513),    # two full passes plus one
          (257, 8)]    # the grand_total fold's second pass
STEPS, FIRST = 9, 7
#: None: a host 0 (below min_replay); else the float32 a training step left on the device
LOSSES = [None, None, 3.25, 0.1, None, 17.0, 1e-3, 2.5e2, None]


@functools.lru_cache(maxsize=None)
def reference(E, N):
    """The rewards and what the restatement holds at each point of the sequence (computed once per shape)."""
    rewards = R.synthetic_rewards(STEPS, E, N, seed=1000 * E + N)
    ref = R.MonitorRef(E, N, report_every=3)
    for t in range(FIRST):
        ref.step(rewards[t], 0 if LOSSES[t] is None else np.float32(LOSSES[t]))
    before_end = ref.episode_reward.copy()
    ref.end_episode()
    avg_at_end = ref.loss.avg
    for t in range(FIRST, STEPS):
        ref.step(rewards[t], 0 if LOSSES[t] is None else np.float32(LOSSES[t]))
    return rewards, ref, before_end, avg_at_end


def feed(mon, rewards, steps):
    import torch
    for t in steps:
        loss = 0 if LOSSES[t] is None else torch.tensor(LOSSES[t], dtype=torch.float32, device="cuda")
        mon.step(torch.from_numpy(rewards[t]).cuda(), loss)


def same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert np.array_equal(R.bits(got), R.bits(want)), what


@pytest.mark.parametrize("E,N", SHAPES)
def test_monitor_equals_the_restatement_bit_for_bit(E, N):
    import torch
    from antsrl_amd.monitor import EpisodeMonitor
    rewards, ref, before_end, avg_at_end = reference(E, N)
    mon = EpisodeMonitor((E, N), report_every=3, max_reports=3, max_episodes=2)
    twin = EpisodeMonitor((E, N), report_every=3, max_reports=3, max_episodes=2)
    feed(mon, rewards, range(FIRST))
    same(mon.episode_reward, before_end, "episode_reward before end_episode")
    assert int(mon.n_losses) == FIRST and mon.n_reports == 2
    mon.end_episode()
    assert not mon.episode_reward.any(), "episode_reward is zero after end_episode"
    same(mon.episode_reward, np.zeros((E, N)), "+0.0, not -0.0")
    same(mon.avg_loss, avg_at_end, "avg_loss carried over")
    feed(mon, rewards, range(FIRST, STEPS))
    same(mon.episode_reward, ref.episode_reward, "episode_reward of the second episode")
    same(mon.avg_loss, ref.loss.avg, "avg_loss")
    same(mon.last_loss, ref.loss.last, "last_loss")
    assert int(mon.n_losses) == STEPS
    log = mon.log()
    for k in range(2):
        for c, name in enumerate(("total", "min", "max")):
            same(log["reports"][k][:, c], ref.reports[k][:, c], "report %d: %s" % (k, name))
    assert list(zip(log["report_episode"], log["report_step"])) == [(0, 3), (0, 6)] == ref.report_at
    total, avg, n = ref.episodes[0]
    same(log["grand_total"], [total], "grand_total")
    same(log["all_loss"], [avg], "all_loss")
    same(log["all_reward"], ref.all_reward, "all_reward")
    assert log["n_losses"].tolist() == [n]
    # two monitors fed the same stream hold equal bits, every word of the block
    feed(twin, rewards, range(FIRST))
    twin.end_episode()
    feed(twin, rewards, range(FIRST, STEPS))
    assert torch.equal(mon._state.view(torch.int64), twin._state.view(torch.int64))


def test_an_episode_without_a_report_logs_zero():
    from antsrl_amd.monitor import EpisodeMonitor
    rewards, _, _, _ = reference(3, 70)
    mon = EpisodeMonitor((3, 70), report_every=50, max_reports=1, max_episodes=2)
    feed(mon, rewards, range(4))
    mon.end_episode()
    log = mon.log()
    assert log["all_reward"].tolist() == [0.0] and len(log["reports"]) == 0 and log["n_losses"].tolist() == [4]


def test_a_step_without_a_loss_leaves_the_running_loss_alone():
    import torch
    from antsrl_amd.monitor import EpisodeMonitor
    rewards, _, _, _ = reference(1, 50)
    mon = EpisodeMonitor((1, 50), report_every=2, max_reports=2, max_episodes=1)
    for t in range(3):
        mon.step(torch.from_numpy(rewards[t]).cuda(), None)
    mon.end_episode()
    log = mon.log()
    assert int(mon.n_losses) == 0 and np.isnan(log["all_loss"][0]) and log["n_losses"].tolist() == [0]
    ref = R.MonitorRef(1, 50, report_every=2)
    for t in range(2):
        ref.step(rewards[t])
    same(log["reports"][0], ref.reports[0], "the report of the second step")


def test_one_report_too_many_raises_and_changes_nothing():
    import ctypes as C
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.monitor import EpisodeMonitor
    rewards, _, _, _ = reference(3, 70)
    mon = EpisodeMonitor((3, 70), report_every=3, max_reports=2, max_episodes=1)
    feed(mon, rewards, range(8))  # reports after the third and the sixth step: the block's two slots
    before = mon._state.clone()
    rw = torch.from_numpy(rewards[8]).cuda()
    with pytest.raises(_lib.AntsrlError, match="max_reports"):
        mon.step(rw, 0.5)           # the ninth step would report
    # the entry itself refuses the slot, before any launch
    rc = _lib.load().antsrl_monitor_step(C.c_void_p(mon._state.data_ptr()), 3, 70, 2, 1, C.c_void_p(rw.data_ptr()), None, 0.5, 1,
                                         2, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"report_slot" in _lib.load().antsrl_last_error()
    torch.cuda.synchronize()
    assert torch.equal(mon._state.view(torch.int64), before.view(torch.int64))
    assert (mon.episode_step, mon.n_reports) == (8, 2)
    mon.end_episode()
    with pytest.raises(_lib.AntsrlError, match="max_episodes"):
        mon.end_episode()
