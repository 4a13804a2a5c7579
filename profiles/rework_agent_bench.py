#!/usr/bin/env python3
"""Times the rework agent's acting step under exploration and its loop (antsrl_amd.agent.ReworkAgent) at
config 5's batch (512 envs x 512 ants, F = 294), float32 and bfloat16 observations, for epsilon in EPSILONS:

  (a) two launches   antsrl_policy_rework over the whole batch, then antsrl_agent_select_actions: the baseline
  (b) fused          antsrl_policy_rework_select, one launch that skips the forward pass of the exploring colonies
  (c) rollout        ReworkAgent.rollout_step with fused_select off and on (K = 4096 rows recorded per step, minibatch
                     264, every step trains), and its parts alone: act, act + select in both forms, record_pre,
                     step_update, record_post, train

Device events around `--iters` calls per case and round; the cases of a group alternate inside a round; five rounds; the
median over the rounds and their spread, (max - min) / median.  The step counter advances with every call, so the
colonies that explore change from call to call as they do in training.  One process.  Prints one line per case and
writes a JSON summary.

    python profiles/rework_agent_bench.py [--iters 200] [--json profiles/rework_agent_c5.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd._lib import ptr as _p  # noqa: E402
from antsrl_amd.agent import ReworkAgent  # noqa: E402
from antsrl_amd.policy import ReworkPolicy  # noqa: E402
from benchlib import E, F, M, N  # noqa: E402

EPSILONS = (0.0, 0.01, 0.1, 0.3, 0.6, 1.0)
FORMATS = ("float32", "bfloat16")
ROUNDS = 5


def rounds(fns, iters):
    """Per fn: (median over ROUNDS of the ms per call, spread of the rounds); the fns alternate inside every round, one
    event pair around `iters` calls of one fn."""
    return BL.median_spread(BL.per_block(fns, iters, rounds=ROUNDS, warmup=5))


def bench_act(fmt, iters):
    """(a) and (b) on synthetic rows (15 % of an observation's values non-zero, as the environment's are sparse)."""
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.rand((E, N, 7, 7, 6), device="cuda", generator=g) * 255.0
    obs[torch.rand(obs.shape, device="cuda", generator=g) >= 0.15] = 0.0
    obs = obs.to(getattr(torch, fmt)).contiguous()
    ast = torch.rand((E, N, 2), device="cuda", generator=g)
    pol = ReworkPolicy(F, "cuda", seed=1)
    rot, ph = (torch.zeros((M,), dtype=torch.int8, device="cuda") for _ in range(2))
    explored = torch.zeros((E,), dtype=torch.uint8, device="cuda")
    step = [0]
    rows = []
    (t_act, s_act), = rounds([lambda: pol.act(obs, ast, out=(rot, ph))], iters)
    for eps in EPSILONS:
        def two():
            step[0] += 1
            pol.act(obs, ast, out=(rot, ph))
            _lib.check(lib.antsrl_agent_select_actions(1, step[0], 0, E, N, eps, 3, 3, _p(rot), _p(ph), _p(explored),
                                                       _lib.stream(pol.device)), "agent_select_actions")

        def fused():
            step[0] += 1
            pol.act_select(obs, ast, seed=1, step=step[0], env_id_base=0, n_envs=E, n_ants=N, epsilon=eps, out=(rot, ph),
                           explored=explored)

        (t2, s2), (t1, s1) = rounds([two, fused], iters)
        rows.append(dict(epsilon=eps, two_launches_ms=t2, two_launches_spread=s2, fused_ms=t1, fused_spread=s1,
                         fused_over_two=t1 / t2))
        print("%-8s eps %-4g  two launches %.4f ms (spread %.1f %%)  fused %.4f ms (spread %.1f %%)  fused / two %.3f"
              % (fmt, eps, t2, 100 * s2, t1, 100 * s1, t1 / t2), flush=True)
    spread = max(max(r["two_launches_spread"], r["fused_spread"]) for r in rows)
    wins = [r["epsilon"] for r in rows if r["fused_ms"] < r["two_launches_ms"] * (1 - spread)]
    return dict(format=fmt, obs_bytes=obs.numel() * obs.element_size(), act_alone_ms=t_act, act_alone_spread=s_act, cases=rows,
                largest_spread=spread,
                fused_wins_from_epsilon=min(wins) if wins and wins == [e for e in EPSILONS if e >= min(wins)] else None)


def c5_env(fmt):
    return BL.c5_env(getattr(torch, fmt))


def agent_on(env, fused, K=4096):
    return BL.warmed(ReworkAgent(epsilon=0.1, record_per_step=K, min_replay=1000, seed=1, fused_select=fused), env)


def bench_rollout(fmt, iters, K=4096):
    env_a, env_b, env_p = c5_env(fmt), c5_env(fmt), c5_env(fmt)
    a, b, p = agent_on(env_a, False, K), agent_on(env_b, True, K), agent_on(env_p, True, K)
    rows = []
    for eps in EPSILONS:
        a.epsilon = b.epsilon = eps
        (t_off, s_off), (t_on, s_on) = rounds([lambda: a.rollout_step(env_a), lambda: b.rollout_step(env_b)], iters)
        rows.append(dict(epsilon=eps, rollout_step_ms=t_off, rollout_step_spread=s_off, rollout_step_fused_ms=t_on,
                         rollout_step_fused_spread=s_on, ant_steps_per_s_fused=M / t_on * 1e3))
        print("%-8s eps %-4g  rollout_step %.4f ms (spread %.1f %%)  fused_select %.4f ms (spread %.1f %%)"
              % (fmt, eps, t_off, 100 * s_off, t_on, 100 * s_on), flush=True)
    # ---- the parts, alone, on a third environment (epsilon 0.3)
    p.epsilon = 0.3
    rot, ph = (t.clone() for t in p.get_action(env_p.obs, env_p.agent_state, False, env=env_p))
    rm, kw = p.replay_memory, p._record_kw()
    idx = torch.randint(0, len(rm), (264,), device="cuda")

    def select_two():
        p.fused_select = False
        p.get_action(env_p.obs, env_p.agent_state, True, env=env_p)

    def select_fused():
        p.fused_select = True
        p.get_action(env_p.obs, env_p.agent_state, True, env=env_p)

    spec = []

    def record_pre():  # (a half timed alone: the ring's "one pre, then one post" bookkeeping is stepped over)
        rm._pending = None
        rm.record_pre(env_p.obs, env_p.agent_state, None, rot.view(-1), ph.view(-1), **kw)
        spec[:] = [rm._pending]

    def record_post():
        rm._pending = spec[0]
        rm.record_post(env_p.obs, env_p.agent_state, None, env_p.reward.view(-1), env_p.done)

    record_pre()
    names = ("act", "act_select_two_launches", "act_select_fused", "record_pre", "step_update", "record_post", "train")
    ts = rounds([lambda: p.get_action(env_p.obs, env_p.agent_state, False, env=env_p), select_two, select_fused, record_pre,
                 lambda: env_p.step_update(rot.view(E, N), ph.view(E, N)), record_post,
                 lambda: p.trainer.step(rm, idx, keep_grads=False)], iters)
    rm._pending = None
    parts = {n: t for n, (t, _) in zip(names, ts)}
    print("%-8s parts at eps 0.3: %s" % (fmt, ", ".join("%s %.4f" % kv for kv in parts.items())), flush=True)
    return dict(format=fmt, shape="512 x 512 ants, 256 x 256 cells", K=K, minibatch=264, cases=rows, parts_epsilon=0.3,
                parts_ms=parts, parts_spread={n: s for n, (_, s) in zip(names, ts)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "rework_agent_c5.json"))
    ap.add_argument("--skip-rollout", action="store_true")
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters, rounds=ROUNDS, envs=E, ants=N, n_features=F,
               act=[bench_act(fmt, args.iters) for fmt in FORMATS])
    if not args.skip_rollout:
        out["rollout"] = [bench_rollout(fmt, max(20, args.iters // 4)) for fmt in FORMATS]
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
