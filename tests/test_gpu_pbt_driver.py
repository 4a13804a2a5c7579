"""driver.train_population(..., pbt=) on the device (antsrl_amd/driver.py, antsrl_amd/pbt.py) for a linear
and a memory population: P = 4 members of Em = 2 colonies of N = 8 ants on 64 x 64 cells, episodes of 12 steps, 16 rows
per member and step against min_replay = 32, so training starts at the second step of episode 0.

1. pbt=None is the loop as it was: nothing of population-based training is constructed, launched or read (no host read
   between an episode's first step and its end), and a run with the argument left out gives the same weights and log.
2. A config with quantile = 0 plans nothing: weights, ring and member_total are pbt=None's, bit for bit; the fitness log
   has a row per generation whose totals are member_total's (the last report is taken at the episode's last step).
3. A real run, quantile 0.5 over three episodes, against a twin driven by hand: episode by episode, pbt_ref on a read of
   episode_reward, pbt_plan with an equally seeded generator, copy_member per kept pair, the hyper-parameters assigned.
   Same weights, targets, Adam moments and ring for every member, same `pbt` log; at least one pair is kept.
   (copy_member is itself an exploit of one pair, so this test holds the LOOP to its rule, not the copy to a second
   implementation: the copy is held against torch copies made tensor by tensor in tests/test_gpu_pbt_exploit.py.)
4. The step after a generation trains with the new learning rates and discounts: the AntsPopSpec handed to the training
   entry carries them."""
import numpy as np
import pytest

import pbt_ref as R
from population_harness import RING

pytestmark = pytest.mark.gpu

P, EM, N, STEPS, EPISODES, SEED = 4, 2, 8, 12, 3, 21
MEMBERS = [dict(epsilon=0.3 + 0.15 * p, discount=0.5 + 0.1 * p, learning_rate=1e-3 * (1 + p), seed=7 + p) for p in range(P)]
KINDS = {
    "linear": ("PopulationAgent", {}, lambda tr: [tr.w1, tr.b1, tr.heads, tr.target_l3, tr._adam]),
    "memory": ("PopulationMemoryAgent", dict(mem_size=3, power=4), lambda tr: [tr._model, tr._target, tr.packed]),
}
BOUNDS = dict(lr_bounds=(1e-5, 1e-2), gap_bounds=(0.01, 0.6))


def fresh(kind):
    """-> (a population of the kind that is not set up, an environment for it, the AntsGen of its maps)."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd import population
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    name, kw, _ = KINDS[kind]
    cfg = cm.make_cfg(P * EM, N, 64, 64, deposit_strength=256.0, max_time=STEPS)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.float32)
    env.reset(synth_init(cfg, seed=5, n_food_discs=6, food_rmin=3, food_rmax=6))
    pop = getattr(population, name)(MEMBERS, replay_size=300, minibatch=16, min_replay=32, update_target_every=2, seed=3, **kw)
    return pop, env, cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)


def state_of(kind, pop):
    """Copies of every member's weights, target, Adam moments (and, for the memory population, pack and memory halves),
    the ring's seven arrays, head and fill, and the counters."""
    tr, ring = pop.trainer, pop.replay_memory
    tensors = KINDS[kind][2](tr) + [getattr(ring, n) for n in RING] + (list(pop._mem) if kind == "memory" else [])
    return [t.clone() for t in tensors], (ring.head, ring.fill, tr.step_count, tr.syncs, tuple(tr.lr), tuple(tr.discount), tuple(pop.epsilon))


def same_state(a, b):
    import torch
    assert a[1] == b[1], (a[1], b[1])
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), i


def same_log(a, b, keys=("reports", "report_episode", "report_step", "grand_total", "member_total", "member_reward", "member_loss",
                         "epsilons")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


_RUNS = {}


def run(kind, mode, pbt_seed=None):
    """One train_population of EPISODES episodes, once per session: mode "left_out" (no pbt argument), "none" (pbt=None,
    with everything of population-based training made to raise and no host read inside an episode), "q0" (quantile 0),
    "real" (quantile 0.5).  -> (log, state_of, the (learning rates, discounts) of the AntsPopSpec of every training step)."""
    key = (kind, mode, pbt_seed)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from antsrl_amd import driver, pbt
    from antsrl_amd.monitor import EpisodeMonitor
    pop, env, gen = fresh(kind)
    env.generate(gen, driver.episode_seed(env.cfg, gen, SEED, 0))  # (train_population generates it again: the same map)
    pop.setup(env)
    tr, specs = pop.trainer, []
    step = tr.step

    def spied(ring, idx, spec=None, loss=None):
        specs.append(([spec.members[p].learning_rate for p in range(P)], [spec.members[p].discount for p in range(P)]))
        return step(ring, idx, spec, loss)
    tr.step = spied
    kw = dict(seed=SEED, report_every=STEPS)
    if mode == "left_out":
        log = driver.train_population(pop, env, gen, EPISODES, STEPS, **kw)
    elif mode == "none":
        mp = pytest.MonkeyPatch()
        fused, end = pop.rollout_step, EpisodeMonitor.end_episode

        def refuse(*a, **k):
            raise AssertionError("pbt=None constructs, launches and reads nothing of population-based training")

        def first_step(e, training=True):
            torch.cuda.set_sync_debug_mode("error")  # from here to the episode's end every host read is an error
            return fused(e, training)

        def end_episode(self):
            end(self)
            torch.cuda.set_sync_debug_mode(0)
        for name in ("PopulationFitness", "pbt_plan", "PbtConfig"):
            mp.setattr(pbt, name, refuse)
        mp.setattr(EpisodeMonitor, "end_episode", end_episode)
        pop.rollout_step, pop.exploit = first_step, refuse
        try:
            log = driver.train_population(pop, env, gen, EPISODES, STEPS, pbt=None, **kw)
        finally:
            torch.cuda.set_sync_debug_mode(0)
            mp.undo()
    else:
        cfg = pbt.PbtConfig(generation_every=1, quantile=0.0 if mode == "q0" else 0.5, seed=pbt_seed or 0, ring=True, **BOUNDS)
        log = driver.train_population(pop, env, gen, EPISODES, STEPS, pbt=cfg, **kw)
    _RUNS[key] = (log, state_of(kind, pop), specs)
    return _RUNS[key]


@pytest.mark.parametrize("kind", list(KINDS))
def test_pbt_none_is_the_loop_as_it_was(kind):
    log, state, specs = run(kind, "none")
    left_log, left_state, _ = run(kind, "left_out")
    assert "pbt" not in log and "pbt" not in left_log
    same_state(state, left_state)
    same_log(log, left_log)
    assert len(specs) == EPISODES * STEPS - 1 and state[1][2] == EPISODES * STEPS - 1  # it trained from episode 0's second step on
    assert all(s == specs[0] for s in specs) and specs[0][0] == [m["learning_rate"] for m in MEMBERS]


@pytest.mark.parametrize("kind", list(KINDS))
def test_quantile_zero_plans_nothing(kind):
    log, state, specs = run(kind, "q0")
    none_log, none_state, none_specs = run(kind, "none")
    same_state(state, none_state)
    same_log(log, none_log)
    assert specs == none_specs
    g = log["pbt"]
    assert g["fitness"].shape == (EPISODES, P, 3) and g["src_of"].tolist() == [list(range(P))] * EPISODES
    assert g["generation_episode"].tolist() == list(range(EPISODES))
    assert g["lr"].shape == g["discount"].shape == (EPISODES + 1, P)
    assert all(np.array_equal(r, [m["learning_rate"] for m in MEMBERS]) for r in g["lr"])
    assert all(np.array_equal(r, [m["discount"] for m in MEMBERS]) for r in g["discount"])
    # the last report is taken at the episode's last step: its totals, summed per member, are the fitness
    assert log["report_step"].tolist() == [STEPS] * EPISODES
    assert np.array_equal(g["fitness"][:, :, 0], log["member_total"]), (g["fitness"][:, :, 0], log["member_total"])
    rep = log["reports"][:, :, 0].reshape(EPISODES, P, EM)
    assert np.array_equal(g["fitness"][:, :, 1], rep.min(axis=2)) and np.array_equal(g["fitness"][:, :, 2], rep.max(axis=2))
    assert len(np.unique(g["fitness"][0, :, 0])) > 1, "the members' rewards do not differ: the real run would rank nothing"


def twin_by_hand(kind):
    """train_population's loop written out, with the generation made by hand.  The plan's seed is chosen after episode 0,
    on the fitness the twin reads there: the first seed whose plan keeps a pair.  -> (seed, the pbt log, state_of)."""
    import torch
    from antsrl_amd import driver
    from antsrl_amd.monitor import EpisodeMonitor
    from antsrl_amd.pbt import pbt_plan
    pop, env, gen = fresh(kind)
    mon = EpisodeMonitor(env, report_every=STEPS, max_reports=EPISODES, max_episodes=EPISODES)
    plan_kw = dict(quantile=0.5, factors=(0.8, 1.25), **BOUNDS)
    seed = rng = None
    env.generate(gen, driver.episode_seed(env.cfg, gen, SEED, 0))  # as run() sets its population up
    pop.setup(env)
    tr = pop.trainer
    out = dict(fitness=[], src_of=[], lr=[tr.lr.copy()], discount=[tr.discount.copy()], generation_episode=[])
    for episode in range(EPISODES):
        env.generate(gen, driver.episode_seed(env.cfg, gen, SEED, episode))
        pop.initialize(env)
        env.observe()
        for s in range(STEPS):
            pop.rollout_step(env, True)
            mon.step(env.reward, None)
        fit = R.fitness(mon.episode_reward.cpu().numpy(), P)
        if rng is None:
            kept = lambda s: (pbt_plan(fit[:, 0], tr.lr, tr.discount, rng=np.random.default_rng(s), **plan_kw)[0] != np.arange(P)).any()  # noqa: E731
            seed = next(s for s in range(64) if kept(s))
            rng = np.random.default_rng(seed)
        src_of, lr, discount = pbt_plan(fit[:, 0], tr.lr, tr.discount, rng=rng, **plan_kw)
        for dst in range(P):
            if src_of[dst] != dst:
                pop.copy_member(int(src_of[dst]), dst, ring=True)
        tr.lr[:], tr.discount[:] = lr, discount
        for k, v in (("fitness", fit), ("src_of", src_of), ("lr", lr), ("discount", discount), ("generation_episode", episode)):
            out[k].append(v)
        mon.end_episode()
        pop.epsilon = [driver.epsilon_schedule(episode, 0.01, 1.0) for _ in range(P)]
    torch.cuda.synchronize()
    return seed, {k: np.array(v) for k, v in out.items()}, state_of(kind, pop)


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_real_run_equals_a_twin_driven_by_hand(kind):
    seed, want, twin_state = twin_by_hand(kind)
    log, state, specs = run(kind, "real", seed)
    g = log["pbt"]
    assert (g["src_of"] != np.arange(P)).any(), "no pair was kept"
    assert (g["src_of"][0] != np.arange(P)).any(), "the seed was chosen so that generation 0 keeps a pair"
    for k in ("fitness", "src_of", "lr", "discount", "generation_episode"):
        assert g[k].dtype == want[k].dtype and g[k].tobytes() == want[k].tobytes(), (k, g[k], want[k])
    same_state(state, twin_state)
    # an inheritor left with its winner's weights ... and trained on: it differs from pbt=None's member
    _, none_state, _ = run(kind, "none")
    assert not all(bool((a == b).all()) for a, b in zip(state[0], none_state[0]))
    # 4. every training step ran with the hyper-parameters of the generations before it
    assert len(specs) == EPISODES * STEPS - 1
    for i, (lr, discount) in enumerate(specs):
        gen_row = (i + 1) // STEPS  # training step i is the loop's step i + 1: episode (i + 1) // STEPS
        assert lr == g["lr"][gen_row].tolist(), (i, lr, g["lr"][gen_row])
        assert discount == np.float32(g["discount"][gen_row]).tolist(), (i, discount, g["discount"][gen_row])
    assert g["lr"][1].tolist() != g["lr"][0].tolist() and specs[STEPS - 1][0] != specs[STEPS - 2][0]
