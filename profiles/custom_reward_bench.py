#!/usr/bin/env python3
"""Times a caller's reward on the device at config 5's batch, 512 envs x 512 ants on 256 x 256 cells:

  coords     k_obs_coords (antsrl_obs_coords): int32 [E][N][7][7][2], 103 MB written per call, as bytes per second — next to
             antsrl_bench_copy (the library's plain 16-byte copy kernel) moving the same number of bytes (half read, half
             written), alternating inside one timed loop.  The coordinates kernel reads 24 bytes per ant and writes 392:
             its bytes are the write.
  give       k_give_reward (antsrl_give_reward) alone: 8 bytes read, 5 written per ant.
  rollout    CollectAgent.rollout_step, bfloat16 observations, K = 4096 rows recorded per step, minibatch 264: un-hooked
             (the device's ExplorationReward) against an env created for a hook (REWARD_NONE, reward_threshold +inf) whose
             hook is written in torch — with the coordinates (an exploration count of its own: a visits map, a gather, a
             scatter) and without them (a reward from agent_state alone) —, alternating in one process.

The method is profiles/explore_agent_bench.py's: device events around warmed iterations that alternate the candidates in
one process, medians; the spread of each (10th and 90th percentile) is reported beside it.  Nothing here is a claim about
a speed-up: the hook is extra work by construction, and the figures say what it costs.

    python profiles/custom_reward_bench.py [--iters 60] [--json profiles/custom_reward_c5.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.agent import CollectAgent  # noqa: E402
from benchlib import M  # noqa: E402


def timed(fns, iters):
    """Per fn in `fns`, [median, 10th percentile, 90th percentile] ms per call, alternating them inside one timed loop."""
    return BL.p50_p10_p90(BL.per_call(fns, iters, 10)).tolist()


def c5_env():
    return BL.c5_env(torch.bfloat16, cm.ACT_CELL_META)


def hook_env():
    """c5_env with the reward left to a hook: REWARD_NONE, and a threshold the kernels' own give_reward never passes."""
    return BL.c5_env(torch.bfloat16, cm.ACT_CELL_META, reward_kind=cm.REWARD_NONE, reward_threshold=float("inf"))


def agent_on(env, K):
    return BL.warmed(CollectAgent(epsilon=0.1, record_per_step=K, min_replay=1000, seed=1, inloop=False), env)


class VisitsHook:
    """An exploration reward of the caller's own, in torch: 0.125 per perceived cell (masked offsets included) nobody of the
    environment has perceived before."""

    def __init__(self, env):
        c = env.cfg
        self.visits = torch.zeros((c.n_envs, c.w, c.h), dtype=torch.bool, device=env.device)
        self.env_of = torch.arange(c.n_envs, device=env.device).view(-1, 1, 1, 1)

    def __call__(self, env, coords, stepped):
        x, y = coords[..., 0].long(), coords[..., 1].long()
        e = self.env_of.expand(x.shape)
        fresh = ~self.visits[e, x, y]
        self.visits[e, x, y] = True
        return fresh.sum(dim=(2, 3)).to(torch.float32) * 0.125


def holding_hook(env, coords, stepped):
    return env.agent_state[..., 0] * 0.5 - 0.25


def bench_kernels(iters):
    env = hook_env()
    env.observe()
    lib = env.lib
    c = env.cfg
    coords = torch.empty((c.n_envs, c.n_ants, c.pside, c.pside, 2), dtype=torch.int32, device=env.device)
    nbytes = coords.numel() * 4
    src = torch.empty((nbytes // 2,), dtype=torch.uint8, device=env.device)
    dst = torch.empty_like(src)
    reward = torch.rand((c.n_envs, c.n_ants), dtype=torch.float64, device=env.device)
    st = lambda: _lib.stream(env.device)  # noqa: E731

    def copy():
        _lib.check(lib.antsrl_bench_copy(_lib.ptr(dst), _lib.ptr(src), nbytes // 2, st()), "bench_copy")
    (t_c, *s_c), (t_cp, *s_cp), (t_g, *s_g) = timed([lambda: env.obs_coords(coords), copy, lambda: env.give_reward(reward, 0.5)], iters)
    return dict(obs_coords_bytes=nbytes, obs_coords_ms=t_c, obs_coords_p10_p90_ms=s_c, obs_coords_GBps=nbytes / t_c * 1e-6,
                copy_bytes_moved=nbytes, copy_ms=t_cp, copy_p10_p90_ms=s_cp, copy_GBps=nbytes / t_cp * 1e-6,
                give_reward_ms=t_g, give_reward_p10_p90_ms=s_g)


def bench_rollout(iters, K=4096):
    envs = [c5_env(), hook_env(), hook_env()]
    envs[1].set_reward_hook(VisitsHook(envs[1]), 0.3)
    envs[2].set_reward_hook(holding_hook, 0.0, coords=False)
    agents = [agent_on(e, K) for e in envs]
    fns = [(lambda a=a, e=e: a.rollout_step(e)) for a, e in zip(agents, envs)]
    (t0, *s0), (t1, *s1), (t2, *s2) = timed(fns, iters)
    return dict(shape="512 x 512 ants, 256 x 256, bf16 observations", K=K, minibatch=264, unhooked_rollout_step_ms=t0,
                unhooked_p10_p90_ms=s0, hooked_coords_rollout_step_ms=t1, hooked_coords_p10_p90_ms=s1,
                hooked_nocoords_rollout_step_ms=t2, hooked_nocoords_p10_p90_ms=s2, coords_hook_over_unhooked_ms=t1 - t0,
                nocoords_hook_over_unhooked_ms=t2 - t0, unhooked_ant_steps_per_s=M / t0 * 1e3,
                hooked_coords_ant_steps_per_s=M / t1 * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "custom_reward_c5.json"))
    ap.add_argument("--skip-rollout", action="store_true")
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters)
    k = out["kernels"] = bench_kernels(args.iters)
    print("k_obs_coords %.4f ms = %.0f GB/s written; antsrl_bench_copy of as many bytes %.4f ms = %.0f GB/s; k_give_reward %.4f ms"
          % (k["obs_coords_ms"], k["obs_coords_GBps"], k["copy_ms"], k["copy_GBps"], k["give_reward_ms"]), flush=True)
    if not args.skip_rollout:
        r = out["rollout"] = bench_rollout(args.iters)
        print("rollout_step un-hooked %.3f ms, hooked with coordinates %.3f ms (+ %.3f), hooked without %.3f ms (+ %.3f)"
              % (r["unhooked_rollout_step_ms"], r["hooked_coords_rollout_step_ms"], r["coords_hook_over_unhooked_ms"],
                 r["hooked_nocoords_rollout_step_ms"], r["nocoords_hook_over_unhooked_ms"]), flush=True)
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
