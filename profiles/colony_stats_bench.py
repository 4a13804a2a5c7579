#!/usr/bin/env python3
"""Times the colony statistics (antsrl_amd.stats.EpisodeStats) at config 5's batch (512 envs x 512 ants,
bfloat16 observations, ReworkAgent) and at config 3's (1024 envs x 512 ants, MemoryAgent), 256 x 256 cells, K = 4096 rows
recorded per step, every step trains:

  (a) loop             50 x (rollout_step, EpisodeMonitor.step): the loop as it is without statistics
  (b) + row            the same 50 steps, then EpisodeStats.record(): a row every 50 steps
  (c) + host path      the same 50 steps, then what a row replaces: antsrl_read_state of the food, explored and pheromone
                       grids and of holding, torch reductions over them on the device, and the results copied to the host
  (d) the row alone    antsrl_stats_row (its two kernels, nothing pending) next to antsrl_bench_copy over the same bytes —
                       the cell records it reads once (a copy of n bytes moves 2 n, so the copy takes half of them)

Device events around a block of 50 steps; the cases alternate inside a round, each on an environment and an agent of its
own; five rounds; the median over the rounds and their spread, (max - min) / median.  One process per batch.

    python profiles/colony_stats_bench.py --config c5 [--json profiles/colony_stats_c5.json]
    python profiles/colony_stats_bench.py --config c3 [--json profiles/colony_stats_c3.json]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.agent import MemoryAgent, ReworkAgent  # noqa: E402
from antsrl_amd.monitor import EpisodeMonitor  # noqa: E402
from antsrl_amd.stats import EpisodeStats  # noqa: E402

EVERY, ROUNDS = 50, 5


def setup(config):
    if config == "c5":
        env = BL.c5_env(torch.bfloat16)
        return env, BL.warmed(ReworkAgent(epsilon=0.1, record_per_step=4096, min_replay=1000, seed=1, fused_select=True), env)
    env = BL.c3_env()  # 20 steps fill the ring past min_replay: every timed step trains
    return env, BL.warmed(MemoryAgent(epsilon=0.1, discount=0.99, learning_rate=1e-5, record_per_step=4096, seed=1), env, steps=20)


def host_path(env):
    """What a row replaces, in its kindest form: the grids stay on the device, torch reduces them, the sums go to the host."""
    food, expl, ph = env.read_state(cm.S_FOOD), env.read_state(cm.S_EXPLORED), env.read_state(cm.S_PHERO)
    hold = env.read_state(cm.S_HOLDING)
    out = (env.read_state(cm.S_TIMESTEP), env.read_state(cm.S_ANTHILL_FOOD), food.sum((1, 2), dtype=torch.float64),
           (food > 0).sum((1, 2)), hold.sum(1, dtype=torch.float64), (hold > 0).sum(1), (expl != 0).sum((1, 2)),
           ph.sum((2, 3), dtype=torch.float64), (ph > 0).sum((2, 3)))
    return [t.cpu() for t in out]


def blocks(fns):
    """Per fn: (median over the rounds of the ms per call, spread); one event pair around one call, the fns alternate."""
    return BL.median_spread(BL.per_block(fns, 1, rounds=ROUNDS, warmup=1))


def bench_loop(config):
    sets = [setup(config) for _ in range(3)]
    mons = [EpisodeMonitor(env, report_every=EVERY, max_reports=64, max_episodes=1) for env, _ in sets]
    stats = EpisodeStats(sets[1][0], max_rows=1)

    def fifty(k):
        env, ag = sets[k]
        for _ in range(EVERY):
            mons[k].step(env.reward, ag.rollout_step(env))

    def loop():
        fifty(0)

    def with_row():
        fifty(1)
        stats.reset()
        stats.record()

    def with_host():
        fifty(2)
        host_path(sets[2][0])

    (t0, s0), (t1, s1), (t2, s2) = blocks([loop, with_row, with_host])
    cfg = sets[0][0].cfg
    print("%s: 50 steps %.3f ms (spread %.1f %%)  + a row %.3f ms (%.1f %%)  + the host path %.3f ms (%.1f %%)"
          % (config, t0, 100 * s0, t1, 100 * s1, t2, 100 * s2), flush=True)
    return dict(envs=cfg.n_envs, ants=cfg.n_ants, cells=[cfg.w, cfg.h], every=EVERY, loop_50_steps_ms=t0, loop_spread=s0,
                with_row_ms=t1, with_row_spread=s1, with_host_path_ms=t2, with_host_path_spread=s2, row_adds_ms=t1 - t0,
                host_path_adds_ms=t2 - t0, row_share_of_50_steps=(t1 - t0) / t0, host_path_share_of_50_steps=(t2 - t0) / t0,
                step_ms=t0 / EVERY), sets[1][0], stats


def bench_alone(env, stats, iters):
    """(d): the row's two kernels with no update pending, and a copy over the bytes of the cell records."""
    lib = _lib.load()
    cfg = env.cfg
    # the bytes a row reads once: the 16-byte records (interleaved layout: scaled units, two pheromones)
    assert cm.uses_scaled_units(cfg) and cfg.n_phero == 2
    rec_bytes = 16 * cfg.n_envs * cfg.w * cfg.h
    a, b = (torch.empty(rec_bytes // 2, dtype=torch.uint8, device=env.device) for _ in range(2))
    st = env._stream()
    env.flush()

    def row():
        for _ in range(iters):
            stats.reset()
            stats.record()

    def copy():
        for _ in range(iters):
            _lib.check(lib.antsrl_bench_copy(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), rec_bytes // 2, st), "bench_copy")

    (tr, sr), (tc, sc) = blocks([row, copy])
    tr, tc = tr / iters, tc / iters
    print("alone: a row %.4f ms (spread %.1f %%) = %.0f GB/s over %.0f MB of records; the copy kernel over the same bytes %.4f "
          "ms (%.1f %%): a row runs at %.2f of its rate" % (tr, 100 * sr, rec_bytes / tr * 1e-6, rec_bytes * 1e-6, tc, 100 * sc, tc / tr),
          flush=True)
    return dict(record_bytes=rec_bytes, row_ms=tr, row_spread=sr, row_gbytes_per_s=rec_bytes / tr * 1e-6, copy_same_bytes_ms=tc,
                copy_spread=sc, fraction_of_copy_rate=tc / tr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("c5", "c3"), default="c5")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--alone", type=int, nargs=3, metavar=("E", "W", "H"), default=None,
                    help="only (d), on a fresh batch of E environments of W x H cells (4 ants): e.g. 16 2048 2048, where a "
                         "segment of the tiled records covers two columns")
    args = ap.parse_args()
    if args.alone:
        from antsrl_amd.batched import BatchedAntsEnv
        from antsrl_amd.synth import synth_init
        E, W, H = args.alone
        cfg = cm.make_cfg(E, 4, W, H, deposit_strength=256.0)
        env = BatchedAntsEnv(cfg)
        env.reset(synth_init(cfg, seed=3))
        out = dict(device=torch.cuda.get_device_name(0), shape=[E, W, H], row_alone=bench_alone(env, EpisodeStats(env, 1), args.iters))
        return BL.write_json(out, args.json)
    loop, env, stats = bench_loop(args.config)
    alone = bench_alone(env, stats, args.iters)
    alone["row_over_step"] = alone["row_ms"] / loop["step_ms"]
    out = dict(device=torch.cuda.get_device_name(0), config=args.config, rounds=ROUNDS, loop=loop, row_alone=alone)
    BL.write_json(out, args.json or os.path.join(ROOT, "profiles", "colony_stats_%s.json" % args.config))


if __name__ == "__main__":
    main()
