"""main.py's episode loop (:66-157) around the device agents' fused step.

    log = train_episodes(agent, env, gen, episodes=100, steps=2000)

runs what the reference's driver runs, on one BatchedAntsEnv handle and without a host read of device data: a fresh map
per episode (antsrl_generate on the same handle), agent.setup once, agent.initialize and the first observation per
episode, `steps` rollout_steps each followed by EpisodeMonitor.step(env.reward, loss), EpisodeMonitor.end_episode, and
the epsilon schedule (:149).  The statistics are the monitor's (antsrl_amd/monitor.py); the one synchronisation is its
log() at the end (and the snapshots, where asked for: a snapshot is a read-back — unless snapshot_on_device keeps the
visualised episodes' frames on the device, antsrl_amd/recorder.py, and reads them once per such episode).  With render_dir
those episodes are also drawn on the device (antsrl_amd/render.py) and written as PNG files.  With stats_every the colony's
own numbers (food at the anthill, on the map and carried, explored cells, pheromone: antsrl_amd/stats.py) are reduced on
the device every so many steps and read back once, with the monitor's log.

`train_population` is the same loop for a PopulationAgent (antsrl_amd/population.py): P linear agents with their own
seed, epsilon, discount and learning rate on one handle, per-member rewards, running losses and epsilon schedules.  It
drives a PopulationExploreAgent unchanged, and `train_population_curriculum` runs the curriculum's two stages for every
member on one handle: the explore population, the hand-over of layer1 on the device, the collect population.
With `pbt=PbtConfig(...)` it is population-based training (antsrl_amd/pbt.py): after a generation's last episode the
members are ranked on the device's fitness row, winners are copied over losers in one launch and the losers' learning
rates and discounts are perturbed; one row read per generation is all the host reads.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np

from . import config as cm
from . import pbt as _pbt
from .monitor import EpisodeMonitor
from .recorder import EpisodeRecorder
from .render import EpisodeRenderer
from .snapshot import snapshot_batched


def epsilon_schedule(episode: int, min_epsilon: float = 0.01, max_epsilon: float = 1.0) -> float:
    """main.py:149: the epsilon set after episode `episode` (counted from 0)."""
    return max(min_epsilon, min(max_epsilon, 1.0 - math.log10((episode + 1) / 2)))


def episode_seed(cfg, gen, seed: int, episode: int) -> int:
    """The seed of episode `episode` under the rule include/antsrl.h documents for auto-reset: + 1 per episode for
    ANTSRL_RNG_COUNTER, + AntsCfg.n_envs_total (0 = env_id_base + n_envs) for ANTSRL_RNG_REFERENCE, so episode k of
    the driver draws the map the k-th auto-reset would have drawn."""
    if gen.rng_kind == cm.RNG_REFERENCE:
        return seed + episode * (cfg.n_envs_total or cfg.env_id_base + cfg.n_envs)
    return seed + episode


def train_population(pop, env, gen, episodes: int, steps: int, *, seed: int = 0, training: bool = True, min_epsilon=0.01,
                     max_epsilon=1.0, monitor: Optional[EpisodeMonitor] = None, report_every: int = 50,
                     save_as: Optional[str] = None, pbt: Optional["_pbt.PbtConfig"] = None) -> dict:
    """train_episodes' loop for a population (antsrl_amd/population.py: PopulationAgent, PopulationExploreAgent,
    PopulationJointAgent, and PopulationMemoryAgent and PopulationReworkAgent, which it drives as they are: the loop reads a population's n_members,
    trainer, epsilon, setup, initialize, rollout_step and save_model and nothing of its net) on `env`, whose
    n_envs are the members' equal shares: a fresh map per episode, pop.setup once, pop.initialize and the first observation per episode, `steps`
    rollout_steps, and after every episode member p's epsilon from epsilon_schedule with its own bounds (min_epsilon,
    max_epsilon: numbers, or arrays [P]).  No host read of device data before the end.

    The statistics per member: its episode reward comes from an EpisodeMonitor's per-environment totals (fed loss=None;
    `monitor` to continue one or by default one that reports every `report_every` steps), summed over the member's
    environments on the host at the end; its running loss is the trainer's `running_loss` (main.py:106-109 from
    the member's first training step on, kept by the training launch), copied into a [episodes, P] device log at each
    episode's end.  save_as: a format with one %d, pop.save_model(p, save_as % p) for every member at the end, when training.

    Returns the monitor's log() with `member_total` and `member_reward` (float64 [episodes, P]: the sum and the mean per
    ant of the member's environments at the episode's last report, 0 without one), `member_loss` (float64 [episodes, P],
    nan while the population has not trained), `epsilons` ([episodes, P]: what each episode ran with) and `monitor`.

    pbt: a PbtConfig (antsrl_amd/pbt.py) turns the fixed sweep into population-based training.  None: nothing of it is
    constructed, launched or read.  With a config, after the last step of every generation_every-th episode and before
    the monitor's end_episode (which zeroes episode_reward): a PopulationFitness row is recorded (antsrl_pop_fitness),
    that ONE row is read back, pbt_plan ranks the members on their totals, pop.exploit copies every winner over its loser
    in one launch (with the ring slab when pbt.ring), and the losers' perturbed learning rates and discounts are
    assigned to pop.trainer.lr / .discount in place.  The read of the row is the one host synchronisation per
    generation: the hyper-parameters travel by value from the host in every launch, so the host has to know who inherited
    what.  The epsilon schedule, the target counter and Adam's step count are common to the members and not touched.
    The log then has `pbt`: dict(fitness [G, P, 3], src_of [G, P], lr and discount [G + 1, P] (row 0: the start),
    generation_episode [G])."""
    import torch
    env = getattr(env, "_backend", env)
    P = pop.n_members
    lo = np.broadcast_to(np.asarray(min_epsilon, dtype=np.float64), (P,))
    hi = np.broadcast_to(np.asarray(max_epsilon, dtype=np.float64), (P,))
    mon = monitor if monitor is not None else EpisodeMonitor(env, report_every=report_every,
                                                             max_reports=max(1, episodes * (steps // report_every)),
                                                             max_episodes=max(1, episodes))
    loss_log = torch.full((max(1, episodes), P), float("nan"), dtype=torch.float64, device=env.device)
    epsilons, first_episode = [], mon.episode  # (a continued monitor counts its earlier episodes)
    fitness = rng = gens = None  # population-based training: made once the population is set up
    for episode in range(episodes):
        env.generate(gen, episode_seed(env.cfg, gen, seed, episode))
        if pop.trainer is None:
            pop.setup(env)
        if pbt is not None and fitness is None:
            fitness = _pbt.PopulationFitness(pop, max_rows=max(1, episodes // pbt.generation_every))
            rng = np.random.default_rng(pbt.seed)
            gens = dict(fitness=[], src_of=[], generation_episode=[],
                        lr=[pop.trainer.lr.copy()], discount=[pop.trainer.discount.copy()])  # row 0: the start
        pop.initialize(env)
        env.observe()
        epsilons.append(pop.epsilon.copy())
        for s in range(steps):
            pop.rollout_step(env, training)
            mon.step(env.reward, None)
        if training and pop.trainer.step_count > 0:
            loss_log[episode].copy_(pop.trainer.running_loss)
        if pbt is not None and (episode + 1) % pbt.generation_every == 0:
            tr = pop.trainer
            row = fitness.row(fitness.record(mon))  # the generation's one host synchronisation
            src_of, lr, discount = _pbt.pbt_plan(row[:, 0], tr.lr, tr.discount, quantile=pbt.quantile, factors=pbt.factors,
                                                 lr_bounds=pbt.lr_bounds, gap_bounds=pbt.gap_bounds, rng=rng)
            dst = np.nonzero(src_of != np.arange(P))[0]
            pop.exploit(src_of[dst], dst, pbt.ring)
            tr.lr[:], tr.discount[:] = lr, discount
            for k, v in dict(fitness=row, src_of=src_of, lr=lr, discount=discount, generation_episode=episode).items():
                gens[k].append(v)
        mon.end_episode()
        pop.epsilon = [epsilon_schedule(episode, float(lo[p]), float(hi[p])) for p in range(P)]
    if save_as is not None and training:
        for p in range(P):
            pop.save_model(p, save_as % p)
    log = mon.log()
    E, N = env.cfg.n_envs, env.cfg.n_ants
    total = np.zeros((episodes, P))
    for episode in range(episodes):
        at = np.nonzero(log["report_episode"] == first_episode + episode)[0]
        if len(at):  # the episode's last report: {total, min, max} per environment
            total[episode] = log["reports"][at[-1], :, 0].reshape(P, E // P).sum(axis=1)
    log.update(member_total=total, member_reward=total / float(E // P * N), member_loss=loss_log[:episodes].cpu().numpy(),
               epsilons=np.array(epsilons).reshape(episodes, P), monitor=mon)
    if pbt is not None:
        gens = gens or dict(fitness=[], src_of=[], generation_episode=[], lr=[], discount=[])  # (a run of no episode)
        log["pbt"] = dict(fitness=np.array(gens["fitness"], dtype=np.float64).reshape(-1, P, 3),
                          src_of=np.array(gens["src_of"], dtype=np.int64).reshape(-1, P),
                          lr=np.array(gens["lr"], dtype=np.float64).reshape(-1, P),
                          discount=np.array(gens["discount"], dtype=np.float64).reshape(-1, P),
                          generation_episode=np.array(gens["generation_episode"], dtype=np.int64))
    return log


def train_population_curriculum(explore_pop, collect_pop, env, gen, episodes, steps: int, *, seed: int = 0,
                                monitor: Optional[EpisodeMonitor] = None, report_every: int = 50, joint_pop=None,
                                **kw) -> tuple:
    """The linear agent's curriculum for every member of a sweep in one process, on one handle and one monitor:
    train_population on `explore_pop` (a PopulationExploreAgent) for episodes[0] episodes, the hand-over on the device
    (collect_pop.setup(env, explore_population=explore_pop): member p's layer1 and layer2 under member p's collect heads),
    then train_population on `collect_pop` (a PopulationAgent of as many members, not set up yet) for episodes[1].
    Stage 2's episode seeds start from seed + episodes[0]; **kw (training, min_epsilon,
    max_epsilon, save_as — a format with one %s for the stage, "explore" or "collect", before the member's %d) goes to
    both stages.  No file round trip, no per-member launch and no host read of device data inside an episode.

    joint_pop (a PopulationJointAgent of as many members, not set up yet): the curriculum's third stage follows, layer1
    trained under the collect heads.  `episodes` then has three entries; the hand-over is
    joint_pop.setup(env, collect_population=collect_pop) (member p's six tensors from member p of stage 2), the episode
    seeds go on from seed + episodes[0] + episodes[1] and save_as's stage name is "joint".

    Returns (stage 1's log, stage 2's log) and, with joint_pop, stage 3's behind them, each train_population's; the
    monitor's rows are shared, so each log holds the reports of the episodes up to its end, and `member_*` and
    `epsilons` are the stage's own."""
    if joint_pop is None:
        e1, e2 = episodes
        e3 = 0
    else:
        e1, e2, e3 = episodes
        assert joint_pop.trainer is None, "the joint population is set up by the hand-over"
        if joint_pop.n_members != collect_pop.n_members:
            raise ValueError("the collect population has %d members, the joint population %d" %
                             (collect_pop.n_members, joint_pop.n_members))
    env = getattr(env, "_backend", env)
    assert collect_pop.trainer is None, "the collect population is set up by the hand-over"
    if explore_pop.n_members != collect_pop.n_members:
        raise ValueError("the explore population has %d members, the collect population %d" %
                         (explore_pop.n_members, collect_pop.n_members))
    mon = monitor if monitor is not None else EpisodeMonitor(env, report_every=report_every,
                                                             max_reports=max(1, (e1 + e2 + e3) * (steps // report_every)),
                                                             max_episodes=max(1, e1 + e2 + e3))
    save_as = kw.pop("save_as", None)
    stage = lambda name: None if save_as is None else save_as % (name, "%d")  # noqa: E731
    if explore_pop.trainer is None:  # (train_population would, at its first episode: e1 = 0 still hands something over)
        env.generate(gen, episode_seed(env.cfg, gen, seed, 0))
        explore_pop.setup(env)
    log1 = train_population(explore_pop, env, gen, e1, steps, seed=seed, monitor=mon, save_as=stage("explore"), **kw)
    collect_pop.setup(env, explore_population=explore_pop)
    log2 = train_population(collect_pop, env, gen, e2, steps, seed=seed + e1, monitor=mon, save_as=stage("collect"), **kw)
    if joint_pop is None:
        return log1, log2
    joint_pop.setup(env, collect_population=collect_pop)
    log3 = train_population(joint_pop, env, gen, e3, steps, seed=seed + e1 + e2, monitor=mon, save_as=stage("joint"), **kw)
    return log1, log2, log3


def train_episodes(agent, env, gen, episodes: int, steps: int, *, seed: int = 0, training: bool = True,
                   min_epsilon: float = 0.01, max_epsilon: float = 1.0, monitor: Optional[EpisodeMonitor] = None,
                   snapshot_every: Optional[int] = None, save_as: Optional[str] = None, snapshot_on_device: bool = False,
                   snapshot_envs=(0,), render_dir: Optional[str] = None, render_every: int = 1,
                   stats_every: Optional[int] = None) -> dict:
    """main.py's loop for `agent` (a device agent: MemoryAgent, CollectAgent, ExploreAgent, ReworkAgent) on `env` (a
    BatchedAntsEnv).  gen: the AntsGen handed to env.generate for every episode (config.make_gen).  An agent that has
    not been set up is set up on `env` at the first episode (once, :82-84).  monitor: an EpisodeMonitor to continue or
    one with another report_every; by default one sized to this run that reports every 50 steps (:115).
    snapshot_every: keep snapshot_batched(env) after every step of episode 0 and of every snapshot_every-th episode
    (:67, :137-138, main.py's visualize_every); those episodes synchronise at every step.  snapshot_on_device: those
    episodes record into an EpisodeRecorder instead (environments snapshot_envs, a block of `steps` frames reused by
    every visualised episode): one launch per step, and one read-back at the episode's end for the same snapshots.
    render_dir (needs snapshot_on_device): after the last step of a visualised episode — the moment main.py pickles —
    every render_every-th recorded frame of the first of snapshot_envs is drawn by an EpisodeRenderer with its defaults
    (a pheromone without max_val is divided by 255, where the recorder's cast saturates) and written to render_dir/episode_%04d/frame_%05d.png.
    save_as: agent.save_model at the end, when training (:154-157).
    stats_every: a row of colony statistics (antsrl_amd/stats.py: food at the anthill, on the map and carried, explored
    cells, pheromone) after step s of an episode when (s + 1) % stats_every == 0, and after an episode's last step if
    that step did not already give one; two launches per row, read back once at the end.  None: nothing is constructed
    and nothing is launched.

    Returns the monitor's log() (reports, report_episode, report_step, all_reward, all_loss, grand_total, n_losses)
    with `epsilons` (the epsilon each episode ran with), `monitor`, `states` (the snapshots, in order) when
    snapshot_every is given, and `stats` when stats_every is: EpisodeStats.rows() plus the host arrays `episode` and
    `step` (counted from 1, as report_step is) of every row.  Not training, all_loss is main.py:111's 0."""
    env = getattr(env, "_backend", env)
    mon = monitor if monitor is not None else EpisodeMonitor(env, report_every=50, max_reports=max(1, episodes * (steps // 50)),
                                                             max_episodes=max(1, episodes))
    if render_dir is not None and not snapshot_on_device:
        raise ValueError("train_episodes: render_dir draws the recorder's frames: it needs snapshot_on_device=True")
    if stats_every is not None and stats_every < 1:
        raise ValueError("train_episodes: stats_every must be >= 1 (%d)" % stats_every)
    states, epsilons = [], []
    recorder = renderer = stats = None
    stats_at = []  # (episode, step) per row; step counts from 1, as the monitor's report_step does
    if stats_every is not None:
        from .stats import EpisodeStats
        stats = EpisodeStats(env, max_rows=max(1, episodes * (steps // stats_every + (1 if steps % stats_every else 0))))
    for episode in range(episodes):
        visualize = snapshot_every is not None and ((episode + 1) % snapshot_every == 0 or episode == 0 or not training)
        env.generate(gen, episode_seed(env.cfg, gen, seed, episode))
        if agent.trainer is None:
            agent.setup(env)
        agent.initialize(env)
        env.observe()
        on_device = visualize and snapshot_on_device
        if on_device:
            if recorder is None:
                recorder = EpisodeRecorder(env, env_indices=snapshot_envs, max_frames=max(1, steps))
            recorder.begin()
        epsilons.append(float(agent.epsilon))
        for s in range(steps):
            loss = agent.rollout_step(env, training)
            mon.step(env.reward, loss if training else None)
            if on_device:
                recorder.record()
            elif visualize:
                states.extend(snapshot_batched(env))
            if stats is not None and ((s + 1) % stats_every == 0 or s == steps - 1):
                stats.record()
                stats_at.append((episode, s + 1))
        if on_device:
            states.extend(recorder.snapshots())
            if render_dir is not None and recorder.n_frames:
                if renderer is None:
                    renderer = EpisodeRenderer(recorder, phero_max_val=None if env.cfg.has_max_val else 255.0)
                renderer.save(os.path.join(render_dir, "episode_%04d" % episode), every=render_every)
        mon.end_episode()
        agent.epsilon = epsilon_schedule(episode, min_epsilon, max_epsilon)
    if save_as is not None and training:
        agent.save_model(save_as)
    log = mon.log()
    if not training:
        log["all_loss"] = np.zeros_like(log["all_loss"])
    log.update(epsilons=np.array(epsilons), monitor=mon)
    if snapshot_every is not None:
        log["states"] = states
    if stats is not None:
        at = np.array(stats_at, dtype=np.int64).reshape(-1, 2)
        log["stats"] = dict(stats.rows(), episode=at[:, 0], step=at[:, 1])
    return log
