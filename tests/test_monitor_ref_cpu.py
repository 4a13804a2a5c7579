"""CPU-side checks of the training monitor: its numpy restatement (tests/monitor_ref.py) against main.py's own arithmetic,
and the C-ABI of antsrl_monitor_* (exported, declared, sized as documented, every bad argument refused before any HIP
call: the pointers below are fakes that are never dereferenced)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import monitor_ref as R
from abi_fakes import FAKE, INVALID, ODD, ODD4, lib  # noqa: F401 (lib is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "antsrl.h")
CONTRACT = os.path.join(HERE, "golden", "contract")
NAMES = ("antsrl_monitor_sizes", "antsrl_monitor_init", "antsrl_monitor_step", "antsrl_monitor_end_episode")


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 50, 70, 255, 256, 257, 513, 4096, 10007])
def test_fold_total_is_a_sum_of_n_float64_adds(n):
    """Any order of n float64 adds stays within gamma_{n-1} * sum |x| of the exact sum, gamma_k = k u / (1 - k u), u = 2^-53
    (the adds of +0.0 the slots start with are exact)."""
    x = R.synthetic_rewards(1, 1, n, seed=n).astype(np.float64).reshape(-1)
    x = x * np.random.default_rng(n).uniform(1.0, 40.0, size=n)  # what an episode_reward holds: not fp32 values
    exact = math.fsum(x.tolist())
    ku = (n - 1) * 2.0 ** -53
    bound = ku * math.fsum(np.abs(x).tolist()) / (1 - ku)
    assert abs(R.fold_total(x) - exact) <= bound
    if n <= 2:  # the order itself, where it can be written out
        assert R.fold_total(x) == (x[0] if n == 1 else x[0] + x[1])


def test_fold_total_order_is_the_documented_one():
    """Written out scalar by scalar: slot t = +0.0 + x[t] + x[t + 256] + ..., then x[i] += x[i + s], s = 128 ... 1."""
    x = R.synthetic_rewards(1, 1, 700, seed=3).astype(np.float64).reshape(-1) * 3.3
    slots = [0.0] * 256
    for t in range(256):
        for n in range(t, len(x), 256):
            slots[t] = slots[t] + float(x[n])
    s = 128
    while s >= 1:
        for i in range(s):
            slots[i] = slots[i] + slots[i + s]
        s //= 2
    assert R.bits(R.fold_total(x)) == R.bits(slots[0])


def test_accumulate_reproduces_the_contract_rewards():
    """F["reward"] of the reference's recorded run, fed step by step: a plain numpy `episode_reward += reward` in every
    bit, as main.py:100 has it (float64 rewards) and as the device has it (float32 rewards)."""
    F = np.load(os.path.join(CONTRACT, "agent_contract.npz"))
    for cast in (np.float64, np.float32):
        rewards = F["reward"].astype(cast)
        mon = R.MonitorRef(1, rewards.shape[1], report_every=5)
        plain = np.zeros(rewards.shape[1])
        for t, r in enumerate(rewards):
            plain += r
            mon.step(r[None, :])
            assert np.array_equal(R.bits(mon.episode_reward[0]), R.bits(plain)), (cast, t)
        assert len(mon.reports) == 2 and mon.report_at == [(0, 5), (0, 10)]
        assert mon.reports[1][0, 1] == plain.min() and mon.reports[1][0, 2] == plain.max()
        assert abs(mon.reports[1][0, 0] - plain.sum()) <= 16 * 2.0 ** -53 * np.abs(plain).sum()
        mon.end_episode()
        assert not mon.episode_reward.any() and mon.all_reward[0] == mon.reports[1][0, 0] / rewards.shape[1]


def test_running_loss_is_main_py_106_109():
    """A literal transcription of main.py:106-109, with the leading host zeros of the steps below min_replay and a first
    non-zero loss behind them."""
    g = np.random.default_rng(5)
    losses = [0, 0, 0] + [np.float32(v) for v in g.uniform(0.01, 30.0, size=40)] + [0] + [np.float32(1e-8), np.float32(3e4)]
    avg_loss = None
    run = R.RunningLoss()
    for loss in losses:
        loss = float(loss)
        if avg_loss is None:
            avg_loss = loss
        else:
            avg_loss = 0.99 * avg_loss + 0.01 * loss
        assert run.update(loss) == avg_loss
    assert run.n == len(losses) and run.last == float(np.float32(3e4)) and avg_loss > 0
    first = R.RunningLoss()
    assert first.avg is None and first.update(np.float32(0.7)) == float(np.float32(0.7))  # the first loss is the average


def test_stale_mean_reward_and_carried_loss():
    """An episode without a report logs 0 (main.py:90), one with reports logs its LAST report; avg_loss carries over."""
    r = R.synthetic_rewards(9, 2, 5, seed=1)
    mon = R.MonitorRef(2, 5, report_every=4)
    for t in range(3):
        mon.step(r[t], 0.5)
    mon.end_episode()
    for t in range(3, 9):
        mon.step(r[t], None)
    mon.end_episode()
    assert mon.all_reward[0] == 0.0 and mon.episodes[0][1:] == (mon.loss.avg, 3)
    er = r[3:7].astype(np.float64).sum(axis=0)  # the report after the second episode's fourth step, not its sixth
    assert np.array_equal(R.bits(mon.reports[0][:, 1]), R.bits(er.min(axis=1)))
    assert mon.all_reward[1] == R.grand_total(mon.reports[0]) / 10.0 and mon.episodes[1][1:] == (mon.loss.avg, 3)


def test_epsilon_schedule_is_main_py_149():
    from antsrl_amd.driver import epsilon_schedule
    min_epsilon, max_epsilon = 0.01, 1
    for episode in range(100):
        want = max(min_epsilon, min(max_epsilon, 1.0 - math.log10((episode + 1) / 2)))
        assert epsilon_schedule(episode) == want == R.epsilon_schedule(episode)
    assert epsilon_schedule(0) == 1 and epsilon_schedule(99) == 0.01 and 0.01 < epsilon_schedule(5) < 1
    assert epsilon_schedule(3, 0.2, 0.5) == 0.5 and epsilon_schedule(99, 0.2, 0.5) == 0.2


def test_episode_seeds_follow_the_auto_reset_rule():
    from antsrl_amd import config as cm
    from antsrl_amd.driver import episode_seed
    cfg = cm.make_cfg(4, 64, 64, 64)
    assert [episode_seed(cfg, cm.make_gen(rng="counter"), 11, k) for k in range(3)] == [11, 12, 13]
    assert [episode_seed(cfg, cm.make_gen(rng="reference"), 11, k) for k in range(3)] == [11, 15, 19]
    shard = cm.make_cfg(4, 64, 64, 64, env_id_base=8, n_envs_total=32)
    assert episode_seed(shard, cm.make_gen(rng="reference"), 11, 2) == 11 + 64


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_and_declared(lib):
    from antsrl_amd import _lib
    text = open(HEADER).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert "int %s(" % name in text, name
    assert "#define ANTSRL_ABI_VERSION 5" in text and lib.antsrl_abi_version() == 5  # additive entries


def test_new_names_are_exported_from_the_package():
    import antsrl_amd
    from antsrl_amd.driver import epsilon_schedule, train_episodes
    from antsrl_amd.monitor import EpisodeMonitor
    assert antsrl_amd.EpisodeMonitor is EpisodeMonitor and antsrl_amd.train_episodes is train_episodes
    assert antsrl_amd.epsilon_schedule is epsilon_schedule
    assert {"EpisodeMonitor", "train_episodes", "epsilon_schedule"} <= set(antsrl_amd.__all__)


def sizes(lib, E, N, R_, P):
    b = C.c_size_t()
    rc = lib.antsrl_monitor_sizes(E, N, R_, P, C.byref(b))
    return rc, b.value


def test_sizes_grow_as_documented(lib):
    for E, N, R_, P in ((1, 1, 1, 1), (1, 50, 40, 100), (3, 70, 2, 1), (257, 8, 4, 3), (512, 512, 8, 2)):
        assert sizes(lib, E, N, R_, P) == (0, 8 * (E * N + 3 + 3 * E * R_ + 3 * P))
    assert sizes(lib, 3, 70, 3, 1)[1] - sizes(lib, 3, 70, 2, 1)[1] == 3 * 3 * 8   # one more report: E rows of 3 doubles
    assert sizes(lib, 3, 70, 2, 2)[1] - sizes(lib, 3, 70, 2, 1)[1] == 3 * 8       # one more episode: one row
    assert sizes(lib, 3, 71, 2, 1)[1] - sizes(lib, 3, 70, 2, 1)[1] == 3 * 8       # one more ant: one double per environment


@pytest.mark.parametrize("dims,msg", [
    ((0, 8, 2, 2), b">= 1"), ((4, 0, 2, 2), b">= 1"), ((4, -1, 2, 2), b">= 1"), ((-4, 8, 2, 2), b">= 1"),
    ((4, 8, 0, 2), b"max_reports"), ((4, 8, 2, 0), b"max_episodes"), ((1 << 16, 1 << 15, 2, 2), b"2^31"),
])
def test_bad_dimensions_are_refused_by_every_entry(lib, dims, msg):
    b = C.c_size_t()
    for rc in (lib.antsrl_monitor_sizes(*dims, C.byref(b)), lib.antsrl_monitor_init(FAKE, *dims, None),
               lib.antsrl_monitor_step(FAKE, *dims, FAKE, None, 0.0, 0, -1, None),
               lib.antsrl_monitor_end_episode(FAKE, *dims, 0, -1, None)):
        assert rc == INVALID and msg in lib.antsrl_last_error(), (dims, lib.antsrl_last_error())


def test_bad_pointers_and_slots_are_refused_without_a_launch(lib):
    d = (4, 8, 2, 3)
    step = lambda state=FAKE, reward=FAKE, loss=None, slot=-1: lib.antsrl_monitor_step(state, *d, reward, loss, 0.0, 1, slot, None)  # noqa: E731
    end = lambda state=FAKE, ep=0, last=-1: lib.antsrl_monitor_end_episode(state, *d, ep, last, None)  # noqa: E731
    for rc, msg in ((lambda: lib.antsrl_monitor_sizes(*d, None), b"NULL bytes"),
                    (lambda: lib.antsrl_monitor_init(None, *d, None), b"NULL state"),
                    (lambda: lib.antsrl_monitor_init(ODD4, *d, None), b"8-byte"),  # 4-byte aligned only
                    (lambda: step(state=None), b"NULL state"), (lambda: step(state=ODD4), b"8-byte"),
                    (lambda: step(reward=None), b"NULL reward"), (lambda: step(reward=ODD), b"4-byte"),
                    (lambda: step(loss=ODD), b"4-byte"),
                    (lambda: step(slot=2), b"report_slot"), (lambda: step(slot=-2), b"report_slot"),
                    (lambda: step(slot=1 << 30), b"report_slot"),
                    (lambda: end(state=None), b"NULL state"), (lambda: end(ep=3), b"episode_slot"),
                    (lambda: end(ep=-1), b"episode_slot"), (lambda: end(last=2), b"last_report_slot"),
                    (lambda: end(last=-2), b"last_report_slot")):
        assert rc() == INVALID and msg in lib.antsrl_last_error(), (msg, lib.antsrl_last_error())
