#!/usr/bin/env python3
"""Times a population of memory agents (antsrl_amd.population.PopulationMemoryAgent) at a sweep's batch:
1024 environments x 512 ants on 256 x 256 cells (config c3's), bfloat16 observations, F = 294, power 5, mem 20, K = 4096
rows recorded per member and step, B = 264, a ring of 20000 rows per member.

  single        a lone MemoryAgent on the whole handle
  population    the population at P = 1, 4, 16 and 64 (--members; member p owns 1024 / P environments of the handle)
  sequential    at P = 4 and 16 (--sequential), P MemoryAgents one after another, each on a shard handle of its own
                environments (the same maps, env_id_base = p Em): the only way there was before, and the yardstick.
                Its rollout_step steps the P shard handles too, as that way has to.

For each: rollout_step, and the stages alone, each as the bare call of its entry through the Python object that owns it:
policy (the forward), select, record (record_pre + record_post of the ring) and train (the trainer's step on fixed
indices).  Every configuration is built and warmed first.  A figure is the time between two device events around
`--steps` consecutive calls, divided by the calls; it is taken `--repeats` times, the configurations alternated inside a
repeat, and reported as the median of the repeats with their spread (max - min), in µs.  The bar: a
difference is called only if it exceeds three times the yardstick's own spread.  Prints one line per configuration and one
JSON line.  Without a GPU it exits with an error.

    python profiles/population_memory_agent_bench.py [--steps 30] [--repeats 3] [--members 1,4,16,64] [--sequential 4,16]
                                                     [--json profiles/population_memory_agent.json]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from benchlib import C3_E as E, C3_N as N, CELLS as W, F  # noqa: E402

POWER, MEM, K, B, RING, MIN_REPLAY = 5, 20, 4096, 264, 20000, 1000
NAMES = ("rollout_step", "policy", "select", "record", "train")


def members(P):
    return BL.members(P, 1e-5)


def make_env(cm, BatchedAntsEnv, n_envs, init, base=0):
    cfg = cm.make_cfg(n_envs, N, W, W, deposit_strength=256.0, act_path=cm.ACT_CELL_META, env_id_base=base, n_envs_total=E)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)
    env.reset({k: np.ascontiguousarray(v[base:base + n_envs]) for k, v in init.items()})
    return env


class Lone:
    """A MemoryAgent on `env` and the five callables of NAMES on it."""

    def __init__(self, env, m, lib):
        from antsrl_amd import _lib
        from antsrl_amd.agent import MemoryAgent
        self.env, self.lib = env, lib
        ag = self.ag = BL.warmed(MemoryAgent(epsilon=m["epsilon"], discount=m["discount"], learning_rate=m["learning_rate"],
                                             record_per_step=K, replay_size=RING, minibatch=B, min_replay=MIN_REPLAY, seed=m["seed"],
                                             mem_size=MEM, power=POWER), env)
        self.rot, self.ph, _ = (t.clone().view(-1) for t in ag.get_action(env.obs, env.agent_state, False, env=env))
        self.idx = torch.randint(0, len(ag.replay_memory), (B,), device=env.device)
        self._p, self._st, self._check = _lib.ptr, _lib.stream(env.device), _lib.check

    def rollout_step(self):
        self.ag.rollout_step(self.env)

    def policy(self):
        ag, env = self.ag, self.env
        ag.policy.act(env.obs, env.agent_state, memory=ag._mem[0], out=ag._mem[1], env=env)

    def select(self):
        ag, p = self.ag, self._p
        self._check(self.lib.antsrl_agent_select(ag.seed, 0, ag.env_id_base, ag.n_envs, ag.n_ants_per_env, float(ag.epsilon), 3, 3, MEM,
                                                 p(self.rot), p(self.ph), p(ag._mem[0]), p(ag._mem[1]), p(ag._explored), self._st),
                    "agent_select")

    def record(self):
        ag, env = self.ag, self.env
        rm = ag.replay_memory
        rm.record_pre(env.obs, env.agent_state, ag._mem[1], self.rot, self.ph, **ag._record_kw())
        rm.record_post(env.obs, env.agent_state, ag._mem[1], env.reward.view(-1), env.done)

    def train(self):
        self.ag.trainer.step(self.ag.replay_memory, self.idx)

    def fns(self):
        return [getattr(self, n) for n in NAMES]


class Sequential:
    """P Lones one after another on their shard handles."""

    def __init__(self, lones):
        self.lones = lones

    def fns(self):
        return [lambda n=n: [getattr(x, n)() for x in self.lones] for n in NAMES]


class Pop:
    """The population on the whole handle and the five callables of NAMES on it."""

    def __init__(self, env, P, lib):
        from antsrl_amd import _lib
        from antsrl_amd.population import PopulationMemoryAgent
        self.env, self.lib = env, lib
        pop = self.pop = BL.warmed(PopulationMemoryAgent(members(P), mem_size=MEM, power=POWER, record_per_step=K, replay_size=RING,
                                                         minibatch=B, min_replay=MIN_REPLAY, seed=1), env)
        self.spec = pop._spec()
        self.idx = torch.randint(0, len(pop.replay_memory), (P, B), device=env.device)
        self._p, self._st, self._check = _lib.ptr, _lib.stream(env.device), _lib.check

    def rollout_step(self):
        self.pop.rollout_step(self.env)

    def policy(self):
        self.pop.get_action(self.env.obs, self.env.agent_state, False, env=self.env, spec=self.spec)

    def select(self):
        pop, p = self.pop, self._p
        self._check(self.lib.antsrl_pop_memory_select(C.byref(self.spec), C.byref(pop.trainer.shape), 0, p(pop._rot), p(pop._ph),
                                                      p(pop._mem[0]), p(pop._mem[1]), p(pop._explored), self._st), "pop_memory_select")

    def record(self):
        pop, env = self.pop, self.env
        rm = pop.replay_memory
        rm.record_pre(env.obs, env.agent_state, pop._mem[1], pop._rot, pop._ph, spec=self.spec, step=0, k=K, shape=pop.trainer.shape)
        rm.record_post(env.obs, env.agent_state, pop._mem[1], env.reward.view(-1), env.done)

    def train(self):
        self.pop.trainer.step(self.pop.replay_memory, self.idx, self.spec)

    def fns(self):
        return [getattr(self, n) for n in NAMES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="consecutive calls between the two events of a figure")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", default="1,4,16,64", help="the population sizes to time")
    ap.add_argument("--sequential", default="4,16", help="of those, the sizes to time one member after another as well")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "population_memory_agent.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("population_memory_agent_bench.py: no GPU: the loop is HIP for gfx950 and has no other form")
    from bench import device_identity
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    sizes, seq_sizes = ([int(x) for x in v.split(",") if x] for v in (args.members, args.sequential))
    assert set(seq_sizes) <= set(sizes), "--sequential names sizes that --members does not"
    lib = _lib.load()
    init = synth_init(cm.make_cfg(E, N, W, W, deposit_strength=256.0, act_path=cm.ACT_CELL_META), seed=3)
    whole = make_env(cm, BatchedAntsEnv, E, init)

    configs = [("single", 1, Lone(whole, members(1)[0], lib))]  # (kind, P, the object with fns())
    for P in sizes:
        configs.append(("population", P, Pop(whole, P, lib)))
        print("built: population P = %d" % P, flush=True)
    for P in seq_sizes:
        Em = E // P
        configs.append(("sequential", P, Sequential([Lone(make_env(cm, BatchedAntsEnv, Em, init, p * Em), m, lib)
                                                     for p, m in enumerate(members(P))])))
        print("built: sequential P = %d" % P, flush=True)
    fns = [c.fns() for _, _, c in configs]
    for f in fns:  # warm-up of every shape: the workspaces, the code objects, the clocks
        for fn in f:
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    # inside a repeat the configurations alternate figure by figure; no warm-up here, so nothing between the one above and
    # the first event: us [configuration][figure][repeat]
    order = [f[j] for j in range(len(NAMES)) for f in fns]
    times = BL.per_block(order, args.steps, rounds=args.repeats, sync_blocks=True) * 1000.0
    times = times.reshape(len(NAMES), len(configs), args.repeats).transpose(1, 0, 2)
    med, spread = BL.median(times), BL.abs_spread(times)

    out = dict(device=device_identity(torch, torch.cuda.current_device()), steps=args.steps, repeats=args.repeats,
               shape="%d x %d ants, %d x %d cells, bf16 observations, F = %d, power %d, mem %d, K = %d per member, B = %d, ring %d rows "
                     "per member" % (E, N, W, W, F, POWER, MEM, K, B, RING),
               figures="us: median over the repeats of (device time of `steps` consecutive calls) / steps; spread_us: max - min "
                       "over the repeats", results=[])
    for i, (kind, P, _) in enumerate(configs):
        r = dict(kind=kind, P=P, us=dict(zip(NAMES, map(float, med[i]))), spread_us=dict(zip(NAMES, map(float, spread[i]))))
        out["results"].append(r)
        print("%-10s P = %2d: %s" % (kind, P, "; ".join("%s %.1f (spread %.1f)" % (n, r["us"][n], r["spread_us"][n]) for n in NAMES)),
              flush=True)
    find = lambda kind, P: next((r for r in out["results"] if r["kind"] == kind and r["P"] == P), None)  # noqa: E731
    claims, single = {}, find("single", 1)
    if find("population", 1):
        one = find("population", 1)
        claims["P1_minus_single_us"] = {n: one["us"][n] - single["us"][n] for n in NAMES}
        claims["P1_within_three_spreads_of_single"] = {n: bool(abs(one["us"][n] - single["us"][n]) <= 3.0 * single["spread_us"][n])
                                                       for n in NAMES}
    for P in seq_sizes:
        pop, seq = find("population", P), find("sequential", P)
        claims["P%d_population_to_sequential" % P] = {n: pop["us"][n] / seq["us"][n] for n in NAMES}
        claims["P%d_below_sequential_by_three_spreads" % P] = {n: bool(pop["us"][n] < seq["us"][n] - 3.0 * seq["spread_us"][n])
                                                               for n in NAMES}
    out["claims"] = claims
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
