#!/usr/bin/env python3
"""Times a population of linear agents (--agent collect: antsrl_amd.population.PopulationAgent), of
explore agents (--agent explore: PopulationExploreAgent), of joint agents (--agent joint:
PopulationJointAgent against CollectAgent(train_layer1=True)) or of rework agents (--agent rework:
PopulationReworkAgent against ReworkAgent; rollout_step acts and selects in one launch in both, the
`policy` and `select` stages are the two entries of the form without the fusion) at config 5's batch: 512 environments x 512 ants
on 256 x 256 cells, bfloat16 observations, K = 4096 rows recorded per member and step, the agent's minibatch (264 / 256).
One environment, stepped by every configuration in turn:

  single        CollectAgent / ExploreAgent / CollectAgent(train_layer1=True) / ReworkAgent alone on the whole batch
  population    the population at P = 1, 4, 16 and 64 (--members; member p owns 512 / P environments)
  sequential    at P = 4 and 16 (--sequential), the same members run one after another on their slices of the batch with
                the single agent's entries (policy, select, record, train: P launches per stage, 2 P for the explore
                and the joint training step): the only way there was before, and the yardstick

For each: rollout_step, and the stages alone, each as the bare call of its entry through the Python object that owns it:
policy (LinearPolicy.act / the population's acting entry), select (antsrl_agent_select_actions / antsrl_pop_select on the
agent's action buffers), record (record_pre + record_post of the ring; DeviceReplayMemory builds its AntsRecordSpec per
call, the population's ring is handed the step's spec) and train (the trainer's step on fixed indices).  hipEvents around
`--iters` warmed iterations, medians; every figure is taken `--repeats` times in the same process and reported as the
median of the repeats with their spread (max - min).  The bar: at P = 16 the population's rollout_step and
its train stage each lie below the sequential run's by more than three times the sequential run's own spread.  Prints one
line per configuration and a JSON summary.

    python profiles/population_bench.py --agent collect|explore|joint|rework [--iters 40] [--repeats 3] [--members 1,4,16,64]
                                        [--sequential 4,16] [--json profiles/population_<agent|explore|joint|rework>_c5.json]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from bench import device_identity  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.agent import CollectAgent, ExploreAgent, ReworkAgent  # noqa: E402
from antsrl_amd.population import PopulationAgent, PopulationExploreAgent, PopulationJointAgent, PopulationReworkAgent  # noqa: E402
from antsrl_amd.replay import DeviceReplayMemory  # noqa: E402
from antsrl_amd.train import ExploreTrainer, JointTrainer, LinearTrainer, ReworkTrainer  # noqa: E402
from benchlib import E, F, N  # noqa: E402

K, RING, MIN_REPLAY = 4096, 20000, 1000
NAMES = ("rollout_step", "policy", "select", "record", "train")
#: per kind: the single agent, the population, the single trainer, whether the net has a pheromone head (without one the
#: environment is stepped and the ring written with None), the minibatch and the default JSON file; single_kw: what the
#: single agent's constructor takes on top
KINDS = dict(collect=dict(single=CollectAgent, population=PopulationAgent, trainer=LinearTrainer, pheromone=True, B=264,
                          json="population_agent_c5.json"),
             explore=dict(single=ExploreAgent, population=PopulationExploreAgent, trainer=ExploreTrainer, pheromone=False, B=256,
                          json="population_explore_c5.json"),
             joint=dict(single=CollectAgent, single_kw=dict(train_layer1=True), population=PopulationJointAgent, trainer=JointTrainer,
                        pheromone=True, B=264, json="population_joint_c5.json"),
             rework=dict(single=ReworkAgent, population=PopulationReworkAgent, trainer=ReworkTrainer, pheromone=True, B=264,
                         json="population_rework_c5.json"))


def timed(fn, iters):
    """Median ms per call of fn (one event pair per call)."""
    return float(BL.median(BL.per_call([fn], iters, 5)[0]))


def figures(fns, iters, repeats):
    """fns: the five callables in NAMES' order -> dict(ms: name -> the median of the repeats' medians, spread_ms: name ->
    their max - min).  A repeat times all five before the next one starts."""
    a = np.array([[timed(fn, iters) for fn in fns] for _ in range(repeats)]).T  # [fn, repeat]
    return dict(ms=dict(zip(NAMES, BL.median(a).tolist())), spread_ms=dict(zip(NAMES, BL.abs_spread(a).tolist())))


def bench_single(kind, env, iters, repeats):
    ag = BL.warmed(kind["single"](epsilon=0.1, record_per_step=K, replay_size=RING, min_replay=MIN_REPLAY, minibatch=kind["B"], seed=1,
                                  **kind.get("single_kw", {})), env)
    rot, ph = (None if t is None else t.clone().view(-1) for t in ag.get_action(env.obs, env.agent_state, False, env=env))
    rm, kw = ag.replay_memory, ag._record_kw()
    idx = torch.randint(0, len(rm), (kind["B"],), device="cuda")

    def rec():
        rm.record_pre(env.obs, env.agent_state, None, rot, ph, **kw)
        rm.record_post(env.obs, env.agent_state, None, env.reward.view(-1), env.done)
    return figures((lambda: ag.rollout_step(env), lambda: ag.policy.act(env.obs, env.agent_state, env=env),
                    lambda: ag._select_actions(0, 3), rec, lambda: ag.trainer.step(rm, idx, keep_grads=False)), iters, repeats)


def members(P):
    return BL.members(P, 1e-4)


def bench_population(kind, env, P, iters, repeats):
    pop = BL.warmed(kind["population"](members(P), record_per_step=K, replay_size=RING, min_replay=MIN_REPLAY, minibatch=kind["B"], seed=1),
                    env)
    rm, spec = pop.replay_memory, pop._spec()
    idx = torch.randint(0, len(rm), (P, kind["B"]), device="cuda")
    ph = pop._ph if kind["pheromone"] else None

    def rec():
        rm.record_pre(env.obs, env.agent_state, None, pop._rot, ph, spec=spec, step=0, k=K)
        rm.record_post(env.obs, env.agent_state, None, env.reward.view(-1), env.done)
    lib, st = _lib.load(), _lib.stream(env.device)

    def select():
        _lib.check(lib.antsrl_pop_select(ctypes.byref(spec), 0, _lib.ptr(pop._rot), _lib.ptr(pop._ph), _lib.ptr(pop._explored), st))
    return dict(P=P, envs_per_member=E // P, train_ms_per_member_step=None,
                **figures((lambda: pop.rollout_step(env), lambda: pop.get_action(env.obs, env.agent_state, False, env=env, spec=spec),
                           select, rec, lambda: pop.trainer.step(rm, idx, spec)), iters, repeats))


class Sequential:
    """P members one after another on their slices of the batch, with the single agent's entries."""

    def __init__(self, kind, env, P):
        self.kind, self.env, self.P, self.Em, self.lib = kind, env, P, E // P, _lib.load()
        self.m = members(P)
        self.tr = [kind["trainer"](F, env.device, discount=m["discount"], lr=m["learning_rate"], seed=m["seed"]) for m in self.m]
        self.rm = [DeviceReplayMemory(RING, (7, 7, 6), [2], [2], device=env.device) for _ in range(P)]
        self.gen = torch.Generator(device=env.device).manual_seed(1)
        self.rot = torch.zeros((E * N,), dtype=torch.int8, device=env.device)
        self.ph = torch.zeros((E * N,), dtype=torch.int8, device=env.device)  # without the head: what select draws, unread
        self.explored = torch.zeros((E,), dtype=torch.uint8, device=env.device)
        self.step = 0

    def rows(self, p):
        return slice(p * self.Em, (p + 1) * self.Em), slice(p * self.Em * N, (p + 1) * self.Em * N)

    def policy(self, copy=True):
        env = self.env
        for p in range(self.P):
            es, ants = self.rows(p)
            rot, ph = self.tr[p].policy.act(env.obs[es], env.agent_state[es], env=env)
            if copy:  # into the batch's action buffers, as the single agent's get_action copies into its own
                self.rot[ants].copy_(rot.reshape(-1))
                if ph is not None:
                    self.ph[ants].copy_(ph.reshape(-1))

    def select(self):
        st = _lib.stream(self.env.device)
        for p, m in enumerate(self.m):
            es, ants = self.rows(p)
            _lib.check(self.lib.antsrl_agent_select_actions(m["seed"], self.step, p * self.Em, self.Em, N, m["epsilon"], 3, 3,
                                                            _lib.ptr(self.rot[ants]), _lib.ptr(self.ph[ants]),
                                                            _lib.ptr(self.explored[es]), st))

    def record_pre(self):
        env = self.env
        for p, m in enumerate(self.m):
            es, ants = self.rows(p)
            self.rm[p].record_pre(env.obs[es], env.agent_state[es], None, self.rot[ants], self.ph[ants] if self.kind["pheromone"] else None,
                                  n_envs=self.Em, n_ants=N, k=K, seed=m["seed"], step=self.step, env_id_base=p * self.Em)

    def record_post(self):
        env = self.env
        for p in range(self.P):
            es, ants = self.rows(p)
            self.rm[p].record_post(env.obs[es], env.agent_state[es], None, env.reward.view(-1)[ants], env.done[es])

    def train(self):
        return [self.tr[p].train(self.rm[p], False, minibatch=self.kind["B"], min_replay=MIN_REPLAY, generator=self.gen)
                for p in range(self.P)]

    def rollout_step(self):
        self.policy()
        self.select()
        self.record_pre()
        self.env.step_update(self.rot.view(E, N), self.ph.view(E, N) if self.kind["pheromone"] else None)
        self.record_post()
        self.step += 1
        return self.train()


def bench_sequential(kind, env, P, iters, repeats):
    s = Sequential(kind, env, P)
    env.set_activation(torch.full((E, N, env.cfg.n_phero), 10.0, device=env.device))
    env.observe()
    for _ in range(3):
        s.rollout_step()
    assert all(t.step_count > 0 for t in s.tr)
    idx = torch.randint(0, len(s.rm[0]), (kind["B"],), device="cuda")

    def rec():
        s.record_pre()
        s.record_post()
    return dict(P=P, **figures((s.rollout_step, lambda: s.policy(copy=False), s.select, rec,
                                lambda: [s.tr[p].step(s.rm[p], idx, keep_grads=False) for p in range(P)]), iters, repeats))


def line(r):
    return "; ".join("%s %.4f (spread %.4f)" % (n, r["ms"][n], r["spread_ms"][n]) for n in NAMES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", choices=sorted(KINDS), required=True)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", default="1,4,16,64", help="the population sizes to time")
    ap.add_argument("--sequential", default="4,16", help="of those, the sizes to time one member after another as well")
    ap.add_argument("--json", default=None, help="default: profiles/population_<agent|explore|joint|rework>_c5.json")
    args = ap.parse_args()
    kind = KINDS[args.agent]
    sizes, seq_sizes = ([int(x) for x in v.split(",") if x] for v in (args.members, args.sequential))
    assert set(seq_sizes) <= set(sizes), "--sequential names sizes that --members does not"
    env = BL.c5_env(torch.bfloat16, cm.ACT_CELL_META)
    out = dict(device=device_identity(torch, torch.cuda.current_device()), agent=args.agent, iters=args.iters, repeats=args.repeats,
               shape="512 x 512 ants, 256 x 256, bf16 observations, K = %d per member, B = %d, ring %d rows per member" % (K, kind["B"], RING),
               figures="ms: median over the repeats of the median of `iters` calls; spread_ms: max - min over the repeats")
    env.observe()
    rot = torch.zeros((E, N), dtype=torch.int8, device=env.device)
    ph = torch.ones_like(rot) if kind["pheromone"] else None
    out["env_step_ms"] = timed(lambda: env.step_update(rot, ph), args.iters)
    out["single"] = bench_single(kind, env, args.iters, args.repeats)
    single = out["single"]["ms"]["rollout_step"]
    print("single %s: %s" % (kind["single"].__name__, line(out["single"])), flush=True)
    out["population"], out["sequential"] = [], []
    for P in sizes:
        r = bench_population(kind, env, P, args.iters, args.repeats)
        r["ratio_to_single"] = r["ms"]["rollout_step"] / single
        r["train_ms_per_member_step"] = r["ms"]["train"] / P  # against the single trainer's step, out["single"]["ms"]["train"]
        out["population"].append(r)
        print("population P = %2d (x %.3f of single): %s" % (P, r["ratio_to_single"], line(r)), flush=True)
    for P in seq_sizes:
        r = bench_sequential(kind, env, P, args.iters, args.repeats)
        pop = next(x for x in out["population"] if x["P"] == P)
        r["ratio_to_single"] = r["ms"]["rollout_step"] / single
        r["population_to_sequential"] = {n: pop["ms"][n] / r["ms"][n] for n in NAMES}
        # the bar: the population below the sequential run by more than three times the sequential run's own spread
        r["below_by_three_spreads"] = {n: bool(pop["ms"][n] < r["ms"][n] - 3.0 * r["spread_ms"][n]) for n in ("rollout_step", "train")}
        out["sequential"].append(r)
        print("sequential P = %2d (population : sequential = %.3f, train %.3f; below by three spreads: %s): %s"
              % (P, r["population_to_sequential"]["rollout_step"], r["population_to_sequential"]["train"],
                 r["below_by_three_spreads"], line(r)), flush=True)
    BL.write_json(out, args.json or os.path.join(ROOT, "profiles", kind["json"]))


if __name__ == "__main__":
    main()
