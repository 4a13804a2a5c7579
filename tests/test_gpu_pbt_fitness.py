"""antsrl_pop_fitness and PopulationFitness on the device (antsrl_popfitness.hip; include/antsrl.h, "Population-based
training") against tests/pbt_ref.py, bit for bit.

1. The kernel at shapes (P, Em, N) that cover one slot, fewer ants than slots, an ant row that crosses the 256 slots once
   and twice, a member whose environments cross the 256 slots, and P at its maximum; on rewards whose sums depend on their
   order (the test asserts that an ascending sum of the same data differs); guard words around `row`; episode_reward is
   left as it was.
2. On a live EpisodeMonitor after a few steps, and PopulationFitness.record twice: two rows."""
from types import SimpleNamespace

import numpy as np
import pytest

import monitor_ref as MR
import pbt_ref as R
from agent_harness import ptr, stream

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 1, 5), (4, 3, 257), (2, 300, 7), (64, 1, 33), (2, 2, 513)]
GUARD = 8  # float64 words in front of and behind `row`
SENTINEL = -7.25e300


def _case(shape):
    P, Em, N = shape
    er = R.ordered_rewards(P, Em, N, seed=1000 * P + 10 * Em + N)
    return er, R.fitness(er, P)


def run_kernel(er, P):
    """-> (row [P, 3] as numpy, the guard words, episode_reward after the call), all read back."""
    import torch
    from antsrl_amd import _lib
    E, N = er.shape
    dev = torch.from_numpy(er).cuda()
    block = torch.full((GUARD + P * 3 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    row = block[GUARD: GUARD + P * 3]
    _lib.check(_lib.load().antsrl_pop_fitness(ptr(dev), E, N, P, ptr(row), stream()), "pop_fitness")
    out = block.cpu().numpy()
    return out[GUARD: GUARD + P * 3].reshape(P, 3), np.concatenate([out[:GUARD], out[GUARD + P * 3:]]), dev.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=["P%d-Em%d-N%d" % s for s in SHAPES])
def test_the_kernel_is_the_reference_bit_for_bit(shape):
    er, want = _case(shape)
    got, guard, after = run_kernel(er, shape[0])
    assert np.array_equal(MR.bits(got), MR.bits(want)), (got, want)
    assert np.array_equal(MR.bits(guard), MR.bits(np.full(2 * GUARD, SENTINEL))), "a word outside row was written"
    assert np.array_equal(MR.bits(after), MR.bits(er)), "episode_reward was written"
    assert (got[:, 1] <= got[:, 2]).all()
    if shape[1] == 1:  # one environment per member: its total is the member's total, min and max
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])


def test_the_data_tells_the_orders_apart():
    """A plain ascending sum of the same rewards differs from the order of sums in at least one shape (in fact in every
    shape with more than a few ants), so an equal row is the ORDER's doing."""
    differ = []
    for shape in SHAPES:
        er, want = _case(shape)
        differ.append(not np.array_equal(MR.bits(R.ascending(er, shape[0])[:, 0]), MR.bits(want[:, 0])))
    assert any(differ), differ
    er, want = _case((2, 300, 7))  # and the member's fold over its environments alone is told apart as well
    totals = np.array([MR.fold_total(r) for r in er]).reshape(2, 300)
    assert any(MR.bits(np.float64(sum(totals[p].tolist()))) != MR.bits(want[p, 0]) for p in range(2))


def test_on_a_live_monitor_and_two_rows():
    """P = 3, Em = 2, N = 300 (an ant row crosses the slots): five steps of synthetic rewards into an EpisodeMonitor, a
    row after step 3 and one after step 5, each the reference on the block's episode_reward at that moment; the monitor's
    block is left alone and its own report of step 5 folds to the same totals."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.monitor import EpisodeMonitor
    from antsrl_amd.pbt import PopulationFitness
    P, Em, N, STEPS = 3, 2, 300, 5
    E = P * Em
    rewards = MR.synthetic_rewards(STEPS, E, N, seed=11)
    mon = EpisodeMonitor((E, N), report_every=STEPS, max_reports=1, max_episodes=1, device="cuda:0")
    fit = PopulationFitness(SimpleNamespace(P=P, n_envs=E, n_ants=N), max_rows=2, device="cuda:0")
    ref = MR.MonitorRef(E, N, report_every=STEPS)
    want = []
    on_device = torch.from_numpy(rewards).to("cuda:0")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # record reads nothing back
    try:
        for s in range(STEPS):
            mon.step(on_device[s])
            ref.step(rewards[s])
            if s in (2, 4):
                assert fit.record(mon) == len(want)
                want.append(R.fitness(ref.episode_reward, P))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert fit.n_rows == 2
    rows = fit.rows()
    assert rows.shape == (2, P, 3) and np.array_equal(MR.bits(rows), MR.bits(np.array(want)))
    assert np.array_equal(MR.bits(fit.row(0)), MR.bits(want[0])) and np.array_equal(MR.bits(fit.row(1)), MR.bits(want[1]))
    assert not np.array_equal(rows[0], rows[1])
    assert np.array_equal(MR.bits(mon.episode_reward.cpu().numpy()), MR.bits(ref.episode_reward))
    rep = mon.log()["reports"][0]  # the report of step 5: the member's total is the grand_total rule on its environments
    assert np.array_equal(MR.bits(rows[1][:, 0]), MR.bits(np.array([MR.fold_total(rep[p * Em:(p + 1) * Em, 0]) for p in range(P)])))
    with pytest.raises(_lib.AntsrlError, match="does not fit max_rows = 2"):
        fit.record(mon)
    other = EpisodeMonitor((E, N + 1), report_every=STEPS, max_reports=1, max_episodes=1, device="cuda:0")
    with pytest.raises(AssertionError):
        PopulationFitness(SimpleNamespace(P=P, n_envs=E, n_ants=N), max_rows=1, device="cuda:0").record(other)
