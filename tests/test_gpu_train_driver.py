"""train_episodes (antsrl_amd/driver.py) against main.py's loop written out by hand: rollout_step, then `.cpu()` of the reward
and the loss at every step, then main.py's arithmetic in numpy and Python floats (:100, :106-109, :115-120, :149-152).

The statistics are equal in every bit (the totals in the order of sums tests/monitor_ref.py restates), the epsilons are
the schedule's, and the trained weights are equal in every bit too: the monitor perturbs nothing."""
import math

import numpy as np
import pytest

import monitor_ref as R
from agent_harness import make_env

pytestmark = pytest.mark.gpu

E, N, STEPS, EPISODES, EVERY, SEED = 4, 64, 12, 3, 5, 21


def the_gen(**kw):
    from antsrl_amd import config as cm
    return cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6, **kw)


def make_agent(kind):
    """Training starts inside the first episode: 256 rows per step against min_replay = 300."""
    from antsrl_amd import agent as A
    kw = dict(epsilon=0.5, learning_rate=1e-3, min_replay=300, replay_size=3000, minibatch=64, seed=7)
    return getattr(A, kind)(**kw)


def stashing_monitor(env, quiet_until_log=False):
    """An EpisodeMonitor that keeps a device copy of episode_reward in front of every end_episode (no read-back); with
    quiet_until_log, log() is where the sync debug mode is lifted."""
    import torch
    from antsrl_amd.monitor import EpisodeMonitor

    class Stash(EpisodeMonitor):
        kept = []

        def end_episode(self):
            self.kept.append(self.episode_reward.clone())
            super().end_episode()

        def log(self):
            if quiet_until_log:
                torch.cuda.set_sync_debug_mode(0)
            return super().log()
    m = Stash(env, report_every=EVERY, max_reports=EPISODES * (STEPS // EVERY), max_episodes=EPISODES)
    m.kept = []
    return m


def hand_loop(agent, env, gen):
    """main.py:66-152 around rollout_step, reading the reward and the loss back at every step."""
    import torch
    from antsrl_amd.driver import episode_seed
    out = dict(episode_reward=[], reports=[], all_loss=[], all_reward=[], epsilons=[], losses=[])
    avg_loss = None
    for episode in range(EPISODES):
        env.generate(gen, episode_seed(env.cfg, gen, SEED, episode))
        if agent.trainer is None:
            agent.setup(env)
        agent.initialize(env)
        env.observe()
        out["epsilons"].append(agent.epsilon)
        episode_reward = np.zeros((E, N))
        last = None
        for s in range(STEPS):
            loss = agent.rollout_step(env)
            reward = env.reward.cpu().numpy()
            loss = float(loss.cpu()) if torch.is_tensor(loss) else loss
            out["losses"].append(loss)
            episode_reward += reward
            if avg_loss is None:
                avg_loss = loss
            else:
                avg_loss = 0.99 * avg_loss + 0.01 * loss
            if (s + 1) % EVERY == 0:
                last = R.report(episode_reward)
                out["reports"].append(last)
        agent.epsilon = max(0.01, min(1, 1.0 - math.log10((episode + 1) / 2)))
        out["all_loss"].append(avg_loss)
        out["all_reward"].append(R.grand_total(last) / float(E * N))
        out["episode_reward"].append(episode_reward)
    return out


def weights(agent):
    t = agent.trainer
    return {k: getattr(t, k) for k in ("model", "target", "heads", "target_l3") if hasattr(t, k)}


@pytest.mark.parametrize("kind", ["ReworkAgent", "CollectAgent", "ExploreAgent"])
def test_the_driver_equals_the_hand_written_loop(kind):
    """ReworkAgent with the agent set up beforehand and every host read an error until log(); CollectAgent and
    ExploreAgent (whose pheromone action is None) set up by the driver."""
    import torch
    from antsrl_amd.driver import epsilon_schedule, train_episodes
    strict = kind == "ReworkAgent"
    env_a, env_b = make_env(E, N, STEPS), make_env(E, N, STEPS)
    a, b = make_agent(kind), make_agent(kind)
    mon = stashing_monitor(env_a, quiet_until_log=strict)
    if strict:
        a.setup(env_a)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
    try:
        log = train_episodes(a, env_a, the_gen(), EPISODES, STEPS, seed=SEED, monitor=mon)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    hand = hand_loop(b, env_b, the_gen())
    assert sum(1 for v in hand["losses"] if v != 0) >= EPISODES * STEPS - 2 and hand["losses"][0] == 0  # host zeros, then training
    for k in range(EPISODES):
        assert np.array_equal(R.bits(mon.kept[k].cpu().numpy()), R.bits(hand["episode_reward"][k])), "episode_reward %d" % k
    assert np.array_equal(R.bits(log["all_loss"]), R.bits(hand["all_loss"]))
    assert np.array_equal(R.bits(log["all_reward"]), R.bits(hand["all_reward"]))
    assert np.array_equal(R.bits(log["reports"]), R.bits(np.stack(hand["reports"])))
    assert list(zip(log["report_episode"], log["report_step"])) == [(e, s) for e in range(EPISODES) for s in (5, 10)]
    assert log["n_losses"].tolist() == [STEPS * (k + 1) for k in range(EPISODES)]
    assert log["epsilons"].tolist() == [0.5] + [epsilon_schedule(k) for k in range(EPISODES - 1)] == hand["epsilons"]
    assert a.epsilon == epsilon_schedule(EPISODES - 1) == b.epsilon
    wa, wb = weights(a), weights(b)
    assert wa and a.trainer.step_count == b.trainer.step_count > 0
    for k in wa:
        assert torch.equal(wa[k].view(torch.int32), wb[k].view(torch.int32)), k  # the monitor perturbs nothing


def test_snapshots_come_from_the_first_and_every_second_episode():
    from antsrl_amd import config as cm
    from antsrl_amd.driver import train_episodes
    env, probe = make_env(E, N, STEPS), make_env(E, N, STEPS)
    log = train_episodes(make_agent("ReworkAgent"), env, the_gen(), EPISODES, STEPS, seed=SEED, snapshot_every=2)
    states = log["states"]
    assert len(states) == 2 * STEPS
    for k, episode in ((0, 0), (STEPS, 1)):
        probe.generate(the_gen(), SEED + episode)
        x, y, r = probe.read_state(cm.S_ANTHILL_XYR).cpu().numpy()[0].tolist()
        for st in states[k: k + STEPS]:
            hill = st.objects[0]
            assert (hill.x, hill.y, hill.radius) == (x, y, r), episode
        assert [st.sim_timestep for st in states[k: k + STEPS]] == list(range(2, STEPS + 2))


def test_episode_k_is_the_map_auto_reset_would_have_drawn():
    """The driver's episode 1 starts from the ants and the anthill of a second handle generated with auto_reset and stepped
    through episode 0 with the same actions (ANTSRL_RNG_COUNTER)."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.driver import train_episodes
    env, other = make_env(E, N, STEPS), make_env(E, N, STEPS)
    agent = make_agent("ReworkAgent")
    acts, start = [], {}
    fused = agent.rollout_step

    def recording(env_, training=True):
        if len(acts) == STEPS:  # the first step of episode 1: the state as generate left it
            start.update(xyt=env_.read_state(cm.S_ANTS_XYT), xyr=env_.read_state(cm.S_ANTHILL_XYR))
        loss = fused(env_, training)
        acts.append((agent._rot.clone(), agent._ph.clone()))
        return loss
    agent.rollout_step = recording
    train_episodes(agent, env, the_gen(), 2, STEPS, seed=SEED)
    other.generate(the_gen(auto_reset=True), SEED)
    for rot, ph in acts[:STEPS]:
        other.step_update(rot.view(E, N), ph.view(E, N))
    assert other.query(cm.Q_TIMESTEP) == 1  # regenerated behind the step that reported done
    assert torch.equal(other.read_state(cm.S_ANTS_XYT), start["xyt"])
    assert torch.equal(other.read_state(cm.S_ANTHILL_XYR), start["xyr"])
