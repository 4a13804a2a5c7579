"""What the benches in this directory share: the two timing loops, the statistics over their samples, the
shapes and warmed setups that make a figure "config 5 with a trainer that trains on every step", and the JSON tail.

The only place in profiles/*.py that creates a timing event (episode_recorder_bench.py keeps one loop of its own: a
host-clock branch and a synchronise before every block).  Both loops return raw samples, ms per call, as a numpy array
whose last axis is the sample axis; a bench applies its statistic to them.

  per_call    one event pair per call, the fns interleaved inside each iteration: linear_agent, explore_agent,
              joint_agent, custom_reward, memory_agent, checkpoint, population, dqn_launch_repeat
  per_block   one event pair around `iters` consecutive calls of one fn, per round: rework_agent, train_driver,
              colony_stats, episode_renderer, memory_train, memory_policy, rework_train, rework_policy,
              population_memory_agent, population_memory_train
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.batched import BatchedAntsEnv  # noqa: E402
from antsrl_amd.synth import synth_init  # noqa: E402

#: config 5's batch: E environments x N ants on CELLS x CELLS cells, F = 7 x 7 x 6 features, M ants in all
E, N, CELLS, F = 512, 512, 256, 294
M = E * N
#: the c3 batch the memory benches use, on the same cells and features
C3_E, C3_N = 1024, 512


def _events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def per_call(fns, iters, warmup):
    """float[len(fns), iters], ms per call: `warmup` times over all fns, a synchronise, then one event pair per call with
    the fns interleaved inside each iteration, and one synchronise at the end."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [_events(iters) for _ in fns]
    for i in range(iters):
        for k, fn in enumerate(fns):
            ev[k][i][0].record()
            fn()
            ev[k][i][1].record()
    torch.cuda.synchronize()
    return np.array([[a.elapsed_time(b) for a, b in row] for row in ev])


def per_block(fns, iters, rounds=1, warmup=0, sync_blocks=False):
    """float[len(fns), rounds], ms per call: `warmup` calls fn by fn and a synchronise (neither with warmup=0: a caller that
    warms up by itself keeps what it had between that and the first event), then per round and fn one event pair around
    `iters` consecutive calls (an int, or one per fn).  A synchronise after every block with sync_blocks, else one at the
    end."""
    iters = [iters] * len(fns) if isinstance(iters, int) else list(iters)
    if warmup:
        for fn in fns:
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
    ev = [_events(rounds) for _ in fns]
    for r in range(rounds):
        for k, fn in enumerate(fns):
            ev[k][r][0].record()
            for _ in range(iters[k]):
                fn()
            ev[k][r][1].record()
            if sync_blocks:
                torch.cuda.synchronize()
    if not sync_blocks:
        torch.cuda.synchronize()
    return np.array([[a.elapsed_time(b) / n for a, b in row] for row, n in zip(ev, iters)])


# ---- statistics over the sample axis (the last one)
def median(t):
    return np.median(t, axis=-1)


def p50_p10_p90(t):
    """[..., 3]: the median, the 10th and the 90th percentile."""
    return np.moveaxis(np.percentile(t, (50, 10, 90), axis=-1), 0, -1)


def abs_spread(t):
    return np.max(t, axis=-1) - np.min(t, axis=-1)


def rel_spread(t):
    return abs_spread(t) / median(t)


def median_spread(t):
    """Per row [(median, relative spread)] as floats: the form the round benches unpack."""
    return list(zip(median(t).tolist(), rel_spread(t).tolist()))


# ---- the warmed setups
def c5_env(obs_dtype, act_path=None, **cfg_kw):
    """Config 5's batch after reset, observations in `obs_dtype`; act_path=None leaves make_cfg's default."""
    if act_path is not None:
        cfg_kw["act_path"] = act_path
    cfg = cm.make_cfg(E, N, CELLS, CELLS, deposit_strength=256.0, **cfg_kw)
    env = BatchedAntsEnv(cfg, obs_dtype=obs_dtype)
    env.reset(synth_init(cfg, seed=3))
    return env


def c3_env():
    cfg = cm.make_cfg(C3_E, C3_N, CELLS, CELLS, deposit_strength=256.0)
    env = BatchedAntsEnv(cfg)
    env.reset(synth_init(cfg, seed=3))
    return env


def warmed(agent, env, steps=3):
    """`agent` set up on `env` and stepped past min_replay: every further rollout_step trains."""
    agent.setup(env)
    agent.initialize(env)
    env.observe()
    for _ in range(steps):
        agent.rollout_step(env)
    assert agent.trainer.step_count > 0
    return agent


def members(P, learning_rate, epsilon=0.1):
    """The hyper-parameters of a sweep's P members; epsilon=None for a trainer alone, which takes none."""
    eps = {} if epsilon is None else dict(epsilon=epsilon)
    return [dict(eps, discount=0.5 + 0.49 * p / max(1, P - 1), learning_rate=learning_rate * (1 + p % 4), seed=1 + p) for p in range(P)]


def write_json(out, path):
    """Writes `out` to `path` (if given) and prints it as the one JSON line."""
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
