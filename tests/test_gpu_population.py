"""PopulationAgent (antsrl_amd/population.py; include/antsrl.h, "The population of linear agents") on the device.

1. The population equals its members: member p is, bit for bit, a CollectAgent's entries run alone on a shard handle of
   its Em environments (env_id_base = p * Em) with the member's own seed, epsilon, discount and learning rate — actions,
   explored flags, rewards and loss after every step; the ring, heads, target layer3, Adam's moments, gradients and
   counters at the end (population_harness.py holds the two shapes and the comparison).
2. copy_member: weights, target, Adam and (optionally) the ring slab of one member over another's.
3. driver.train_population: per-member rewards, running losses and epsilons, with no host read inside an episode."""
import numpy as np
import pytest

from population_harness import COLLECT as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_population_equals_its_members(name):
    import torch
    s = H.SHAPES[name]
    run = H.checked_run(name)  # every comparison of the module docstring's point 1 is made in there
    end, P, Em = run.final, s["P"], s["Em"]
    explored = torch.stack([w.explored for w in run.log]).cpu().numpy().reshape(s["steps"], P, Em)
    for p in range(P):
        if s["epsilon"][p] == 0.0:
            assert not explored[:, p].any(), "member %d has epsilon 0 and explored" % p
        if s["epsilon"][p] == 1.0:
            assert explored[:, p].all(), "member %d has epsilon 1 and did not always explore" % p
    assert end.step_count >= 8 and end.syncs >= 1, (end.step_count, end.syncs)
    k = s["K"] or Em * s["N"]
    assert end.fill == s["ring"] and end.head == (k * s["steps"]) % s["ring"]  # the ring wrapped
    # members that share a seed differ through their environment ids (and members at large differ at all)
    rot = torch.stack([w.rot for w in run.log]).view(s["steps"], P, -1)
    for p in range(P):
        for q in range(p + 1, P):
            assert not torch.equal(rot[:, p], rot[:, q]), (p, q)
            assert not torch.equal(end.heads[p], end.heads[q]), (p, q)
    losses = torch.stack([w.loss for w in run.log if torch.is_tensor(w.loss)])
    assert losses.shape == (end.step_count, P) and bool(torch.isfinite(losses).all())


def test_copy_member():
    tr = H.checked_run("a").pop.trainer
    weights = lambda p: [t[p].clone() for t in (tr.w1, tr.b1, tr.heads, tr.target_l3, tr._adam)]  # noqa: E731
    H.check_copy_member(weights, "weights, target and Adam are member 0's")  # the assertions are the harness's


def test_train_population(monkeypatch):
    """P = 2, Em = 1, 32 ants, 2 episodes of 10 steps; 32 rows per step against min_replay = 96: training starts at step 3."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.driver import epsilon_schedule, train_population
    from antsrl_amd.monitor import EpisodeMonitor
    from antsrl_amd.population import PopulationAgent
    P, N, EPISODES, STEPS = 2, 32, 2, 10
    env, _ = H.make_envs(P, 1, N, STEPS, False)
    pop = PopulationAgent([dict(epsilon=0.5, discount=0.5, learning_rate=1e-3, seed=7),
                           dict(epsilon=0.9, discount=0.99, learning_rate=1e-4, seed=9)],
                          replay_size=300, minibatch=32, min_replay=96, seed=3)
    fused, end = pop.rollout_step, EpisodeMonitor.end_episode
    seen = []

    def step(e, training=True):
        torch.cuda.set_sync_debug_mode("error")  # from here to the episode's end every host read is an error
        loss = fused(e, training)
        seen.append((e.reward.clone(), loss))
        return loss

    def end_episode(self):
        end(self)
        torch.cuda.set_sync_debug_mode(0)
    pop.rollout_step = step
    monkeypatch.setattr(EpisodeMonitor, "end_episode", end_episode)
    gen = cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)
    lo, hi = np.array([0.01, 0.3]), np.array([1.0, 0.6])
    try:
        log = train_population(pop, env, gen, EPISODES, STEPS, seed=21, min_epsilon=lo, max_epsilon=hi, report_every=STEPS)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    monkeypatch.undo()
    assert len(seen) == EPISODES * STEPS
    assert [torch.is_tensor(l) for _, l in seen[:STEPS]] == [False, False] + [True] * (STEPS - 2), "training starts at step 3"
    assert pop.trainer.step_count == EPISODES * STEPS - 2
    # the epsilons: what each episode ran with, member by member
    want_eps = [[0.5, 0.9], [epsilon_schedule(0, lo[0], hi[0]), epsilon_schedule(0, lo[1], hi[1])]]
    assert np.array_equal(log["epsilons"], np.array(want_eps)) and want_eps[1] == [1.0, 0.6]
    assert list(pop.epsilon) == [epsilon_schedule(1, lo[p], hi[p]) for p in range(P)]
    # per member: an EpisodeMonitor of its own environment, fed its rewards and (from its first training step on) its losses
    for p in range(P):
        mon = EpisodeMonitor((1, N), report_every=STEPS, max_reports=EPISODES, max_episodes=EPISODES, device=env.device)
        for i, (reward, loss) in enumerate(seen):
            mon.step(reward[p:p + 1].contiguous(), loss[p:p + 1] if torch.is_tensor(loss) else None)
            if (i + 1) % STEPS == 0:
                mon.end_episode()
        ref = mon.log()
        assert np.array_equal(log["member_total"][:, p], ref["grand_total"]), (p, log["member_total"][:, p], ref["grand_total"])
        assert np.array_equal(log["member_reward"][:, p], ref["all_reward"]), p
        assert np.array_equal(log["member_loss"][:, p], ref["all_loss"]), (p, log["member_loss"][:, p], ref["all_loss"])
        assert np.isfinite(log["member_loss"][:, p]).all() and ref["n_losses"][-1] == EPISODES * STEPS - 2
    assert not np.array_equal(log["member_loss"][:, 0], log["member_loss"][:, 1])
    assert np.array_equal(log["member_total"].sum(axis=1), log["reports"][:, :, 0].sum(axis=1))
