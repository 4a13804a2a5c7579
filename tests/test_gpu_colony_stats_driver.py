"""train_episodes(..., stats_every=5) (antsrl_amd/driver.py): ReworkAgent, 2 episodes of 12 steps, 3 environments of 64
ants.  Rows come after the steps 5, 10 and 12 of each episode and the log's `episode` / `step` say so; they equal, in
every bit, the rows of a hand-written loop that takes antsrl_read_state at those steps and feeds it to tests/stats_ref.py;
and the same run without stats_every returns the same rewards, losses and epsilons, and no "stats" key."""
import numpy as np
import pytest

import monitor_ref as R
import stats_ref as S
from agent_harness import make_env

pytestmark = pytest.mark.gpu

E, N, STEPS, EPISODES, SEED, EVERY = 3, 64, 12, 2, 21, 5
AT = [(ep, s) for ep in range(EPISODES) for s in (5, 10, 12)]


def the_gen():
    from antsrl_amd import config as cm
    return cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)


def make_agent():
    """Training starts inside the first episode: 192 rows per step against min_replay = 300."""
    from antsrl_amd.agent import ReworkAgent
    return ReworkAgent(epsilon=0.5, learning_rate=1e-3, min_replay=300, replay_size=3000, minibatch=64, seed=7)


def by_hand():
    """The driver's loop, written out, with a read_state look where the driver takes a row."""
    from antsrl_amd import config as cm
    from antsrl_amd.driver import episode_seed, epsilon_schedule
    env, agent, gen = make_env(E, N, STEPS), make_agent(), the_gen()
    which = dict(timestep=cm.S_TIMESTEP, anthill_food=cm.S_ANTHILL_FOOD, food=cm.S_FOOD, holding=cm.S_HOLDING,
                 explored=cm.S_EXPLORED, phero=cm.S_PHERO)
    rows = []
    for episode in range(EPISODES):
        env.generate(gen, episode_seed(env.cfg, gen, SEED, episode))
        if agent.trainer is None:
            agent.setup(env)
        agent.initialize(env)
        env.observe()
        for s in range(STEPS):
            agent.rollout_step(env, True)
            if (episode, s + 1) in AT:
                rows.append(S.rows({k: env.read_state(w).cpu().numpy() for k, w in which.items()}, env.cfg))
        agent.epsilon = epsilon_schedule(episode)
    return np.stack(rows), env.cfg


def test_the_drivers_rows_are_the_rows_of_a_loop_with_read_state():
    from antsrl_amd.driver import train_episodes
    log = train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), EPISODES, STEPS, seed=SEED, stats_every=EVERY)
    plain = train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), EPISODES, STEPS, seed=SEED)
    st = log["stats"]
    assert list(zip(st["episode"].tolist(), st["step"].tolist())) == AT
    want, cfg = by_hand()
    ref = S.decode(want, cfg.n_phero)
    assert sorted(ref) == sorted(k for k in st if k not in ("episode", "step"))
    for k in ref:
        assert st[k].shape == ref[k].shape == ((len(AT), E, cfg.n_phero) if k.startswith("phero") else (len(AT), E)), k
        assert st[k].dtype == ref[k].dtype and np.array_equal(st[k].view(np.int64), ref[k].view(np.int64)), k
    assert st["timestep"].tolist() == [[s + 1] * E for _, s in AT]
    assert (st["phero_cells"].sum(axis=2) > 0).all() and (st["explored_cells"][2] > st["explored_cells"][0]).all()  # the rows say something
    # ---- without stats_every: the same run, and no key
    assert "stats" not in plain
    for k in ("reports", "all_reward", "all_loss", "grand_total", "epsilons"):
        assert np.array_equal(R.bits(log[k]), R.bits(plain[k])), k
    for k in ("report_episode", "report_step", "n_losses"):
        assert np.array_equal(log[k], plain[k]), k
    assert int(log["n_losses"][-1]) > 0  # (training ran)


def test_a_row_at_the_last_step_is_not_taken_twice_and_a_bad_cadence_is_refused():
    from antsrl_amd.driver import train_episodes
    log = train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), 1, 6, seed=SEED, stats_every=3)
    assert log["stats"]["step"].tolist() == [3, 6] and log["stats"]["episode"].tolist() == [0, 0]
    with pytest.raises(ValueError, match="stats_every"):
        train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), 1, 6, seed=SEED, stats_every=0)
