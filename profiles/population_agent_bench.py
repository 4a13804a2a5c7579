#!/usr/bin/env python3
"""Times a population of linear agents (antsrl_amd.population.PopulationAgent) at config 5's batch: 512
environments x 512 ants on 256 x 256 cells, bfloat16 observations, K = 4096 rows recorded per member and step, minibatch
264.  One environment, stepped by every configuration in turn:

  single        CollectAgent alone on the whole batch (today's agent)
  population    PopulationAgent at P = 1, 4, 16 and 64 (member p owns 512 / P environments)
  sequential    at P = 4 and 16, the same members run one after another on their slices of the batch with the single
                agent's entries (policy, select, record, train: P launches per stage): the only way there was before

For each: rollout_step, and the stages alone, each as the bare call of its entry through the Python object that owns it:
policy (LinearPolicy.act / antsrl_pop_policy), select (antsrl_agent_select_actions / antsrl_pop_select on the agent's
action buffers), record (record_pre + record_post of the ring; DeviceReplayMemory builds its AntsRecordSpec per call, the
population's ring is handed the step's spec) and train (the trainer's step on fixed indices).  hipEvents around `--iters`
warmed iterations, medians.  Prints one line per configuration and a JSON summary.

    python profiles/population_agent_bench.py [--iters 40] [--json profiles/population_agent_c5.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import device_identity  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.agent import CollectAgent  # noqa: E402
from antsrl_amd.batched import BatchedAntsEnv  # noqa: E402
from antsrl_amd.population import PopulationAgent  # noqa: E402
from antsrl_amd.replay import DeviceReplayMemory  # noqa: E402
from antsrl_amd.synth import synth_init  # noqa: E402
from antsrl_amd.train import LinearTrainer  # noqa: E402

E, N, F, K, B, RING, MIN_REPLAY = 512, 512, 294, 4096, 264, 20000, 1000


def timed(fn, iters, warmup=5):
    """Median ms per call of fn (one event pair per call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def stages(policy, select, record, train, iters):
    return dict(policy=timed(policy, iters), select=timed(select, iters), record=timed(record, iters), train=timed(train, iters))


def bench_single(env, iters):
    ag = CollectAgent(epsilon=0.1, record_per_step=K, replay_size=RING, min_replay=MIN_REPLAY, minibatch=B, seed=1)
    ag.setup(env)
    ag.initialize(env)
    env.observe()
    for _ in range(3):
        ag.rollout_step(env)  # past min_replay: every further step trains
    step = timed(lambda: ag.rollout_step(env), iters)
    rot, ph = (t.clone() for t in ag.get_action(env.obs, env.agent_state, False, env=env))
    rm, kw = ag.replay_memory, ag._record_kw()
    idx = torch.randint(0, len(rm), (B,), device="cuda")

    def rec():
        rm.record_pre(env.obs, env.agent_state, None, rot.view(-1), ph.view(-1), **kw)
        rm.record_post(env.obs, env.agent_state, None, env.reward.view(-1), env.done)
    return dict(rollout_step_ms=step, stages_ms=stages(lambda: ag.policy.act(env.obs, env.agent_state, env=env),
                                                       lambda: ag._select_actions(0, 3), rec,
                                                       lambda: ag.trainer.step(rm, idx, keep_grads=False), iters))


def members(P):
    return [dict(epsilon=0.1, discount=0.5 + 0.49 * p / max(1, P - 1), learning_rate=1e-4 * (1 + p % 4), seed=1 + p) for p in range(P)]


def bench_population(env, P, iters):
    pop = PopulationAgent(members(P), record_per_step=K, replay_size=RING, min_replay=MIN_REPLAY, minibatch=B, seed=1)
    pop.setup(env)
    pop.initialize(env)
    env.observe()
    for _ in range(3):
        pop.rollout_step(env)
    assert pop.trainer.step_count > 0
    step = timed(lambda: pop.rollout_step(env), iters)
    rm, spec = pop.replay_memory, pop._spec()
    idx = torch.randint(0, len(rm), (P, B), device="cuda")

    def rec():
        rm.record_pre(env.obs, env.agent_state, None, pop._rot, pop._ph, spec=spec, step=0, k=K)
        rm.record_post(env.obs, env.agent_state, None, env.reward.view(-1), env.done)
    lib, st = _lib.load(), _lib.stream(env.device)

    def select():
        _lib.check(lib.antsrl_pop_select(ctypes.byref(spec), 0, _lib.ptr(pop._rot), _lib.ptr(pop._ph), _lib.ptr(pop._explored), st))
    return dict(P=P, envs_per_member=E // P, rollout_step_ms=step,
                stages_ms=stages(lambda: pop.get_action(env.obs, env.agent_state, False, env=env, spec=spec), select, rec,
                                 lambda: pop.trainer.step(rm, idx, spec), iters))


class Sequential:
    """P members one after another on their slices of the batch, with the single agent's entries."""

    def __init__(self, env, P):
        self.env, self.P, self.Em, self.lib = env, P, E // P, _lib.load()
        self.m = members(P)
        self.tr = [LinearTrainer(F, env.device, discount=m["discount"], lr=m["learning_rate"], seed=m["seed"]) for m in self.m]
        self.rm = [DeviceReplayMemory(RING, (7, 7, 6), [2], [2], device=env.device) for _ in range(P)]
        self.gen = torch.Generator(device=env.device).manual_seed(1)
        self.rot = torch.zeros((E * N,), dtype=torch.int8, device=env.device)
        self.ph = torch.zeros((E * N,), dtype=torch.int8, device=env.device)
        self.explored = torch.zeros((E,), dtype=torch.uint8, device=env.device)
        self.step = 0

    def rows(self, p):
        return slice(p * self.Em, (p + 1) * self.Em), slice(p * self.Em * N, (p + 1) * self.Em * N)

    def policy(self, copy=True):
        env = self.env
        for p in range(self.P):
            es, ants = self.rows(p)
            rot, ph = self.tr[p].policy.act(env.obs[es], env.agent_state[es], env=env)
            if copy:  # into the batch's action buffers, as CollectAgent.get_action copies into its own
                self.rot[ants].copy_(rot.reshape(-1))
                self.ph[ants].copy_(ph.reshape(-1))

    def select(self):
        st = _lib.stream(self.env.device)
        for p, m in enumerate(self.m):
            es, ants = self.rows(p)
            _lib.check(self.lib.antsrl_agent_select_actions(m["seed"], self.step, p * self.Em, self.Em, N, m["epsilon"], 3, 3,
                                                            _lib.ptr(self.rot[ants]), _lib.ptr(self.ph[ants]),
                                                            _lib.ptr(self.explored[es]), st))

    def act(self):
        self.policy()
        self.select()

    def record_pre(self):
        env = self.env
        for p, m in enumerate(self.m):
            es, ants = self.rows(p)
            self.rm[p].record_pre(env.obs[es], env.agent_state[es], None, self.rot[ants], self.ph[ants], n_envs=self.Em, n_ants=N,
                                  k=K, seed=m["seed"], step=self.step, env_id_base=p * self.Em)

    def record_post(self):
        env = self.env
        for p in range(self.P):
            es, ants = self.rows(p)
            self.rm[p].record_post(env.obs[es], env.agent_state[es], None, env.reward.view(-1)[ants], env.done[es])

    def train(self):
        return [self.tr[p].train(self.rm[p], False, minibatch=B, min_replay=MIN_REPLAY, generator=self.gen) for p in range(self.P)]

    def rollout_step(self):
        self.act()
        self.record_pre()
        self.env.step_update(self.rot.view(E, N), self.ph.view(E, N))
        self.record_post()
        self.step += 1
        return self.train()


def bench_sequential(env, P, iters):
    s = Sequential(env, P)
    env.set_activation(torch.full((E, N, env.cfg.n_phero), 10.0, device=env.device))
    env.observe()
    for _ in range(3):
        s.rollout_step()
    assert all(t.step_count > 0 for t in s.tr)
    step = timed(s.rollout_step, iters)
    idx = torch.randint(0, len(s.rm[0]), (B,), device="cuda")

    def rec():
        s.record_pre()
        s.record_post()
    return dict(P=P, rollout_step_ms=step,
                stages_ms=stages(lambda: s.policy(copy=False), s.select, rec,
                                 lambda: [s.tr[p].step(s.rm[p], idx, keep_grads=False) for p in range(P)], iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "population_agent_c5.json"))
    args = ap.parse_args()
    cfg = cm.make_cfg(E, N, 256, 256, deposit_strength=256.0, act_path=cm.ACT_CELL_META)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)
    env.reset(synth_init(cfg, seed=3))
    ph = torch.ones((E, N), dtype=torch.int8, device=env.device)
    out = dict(device=device_identity(torch, torch.cuda.current_device()), iters=args.iters,
               shape="512 x 512 ants, 256 x 256, bf16 observations, K = %d per member, B = %d, ring %d rows per member" % (K, B, RING))
    env.observe()
    rot = torch.zeros_like(ph)
    out["env_step_ms"] = timed(lambda: env.step_update(rot, ph), args.iters)
    out["single"] = bench_single(env, args.iters)
    print("single CollectAgent: rollout_step %.3f ms; %s" % (out["single"]["rollout_step_ms"], out["single"]["stages_ms"]), flush=True)
    out["population"], out["sequential"] = [], []
    for P in (1, 4, 16, 64):
        r = bench_population(env, P, args.iters)
        r["ratio_to_single"] = r["rollout_step_ms"] / out["single"]["rollout_step_ms"]
        out["population"].append(r)
        print("population P = %2d: rollout_step %.3f ms (x %.3f of single); %s" % (P, r["rollout_step_ms"], r["ratio_to_single"], r["stages_ms"]), flush=True)
    for P in (4, 16):
        r = bench_sequential(env, P, args.iters)
        pop = next(x for x in out["population"] if x["P"] == P)
        r["population_to_sequential"] = pop["rollout_step_ms"] / r["rollout_step_ms"]
        r["agent_stages_population_to_sequential"] = sum(pop["stages_ms"].values()) / sum(r["stages_ms"].values())
        out["sequential"].append(r)
        print("sequential P = %2d: rollout_step %.3f ms (population : sequential = %.3f; agent stages alone %.3f); %s"
              % (P, r["rollout_step_ms"], r["population_to_sequential"], r["agent_stages_population_to_sequential"], r["stages_ms"]), flush=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
