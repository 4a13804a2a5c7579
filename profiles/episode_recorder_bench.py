#!/usr/bin/env python3
"""Times a visualised episode's step (antsrl_amd.recorder.EpisodeRecorder) at config 5's batch (512 envs x 512
ants, 256 x 256 cells, bfloat16 observations, ReworkAgent, K = 4096 rows recorded per step, every step trains):

  (a) step              ReworkAgent.rollout_step, then EpisodeMonitor.step(env.reward, loss)
  (b) + record          the same, then EpisodeRecorder.record() of environment 0: one launch, nothing read back
  (c) + flush           the same as (a), then antsrl_flush alone: what of (b) is the update leaving k_update_move
  (d) + snapshot        the same as (a), then snapshot.snapshot_batched(env): the path the recorder replaces — the state of
                        all environments through antsrl_read_state and .cpu(), a synchronisation per array

(a)-(c): device events around `--iters` calls per case and round.  (d) synchronises the host in every call, so it is timed
by the host's clock between two device synchronisations, over `--snapshot-iters` calls.  The cases alternate inside a
round; five rounds; the median over the rounds and their spread, (max - min) / median (profiles/train_driver_bench.py's
method).  One process.

    python profiles/episode_recorder_bench.py [--iters 100] [--snapshot-iters 10] [--json profiles/episode_recorder_c5.json]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd.agent import ReworkAgent  # noqa: E402
from antsrl_amd.monitor import EpisodeMonitor  # noqa: E402
from antsrl_amd.recorder import EpisodeRecorder  # noqa: E402
from antsrl_amd.snapshot import snapshot_batched  # noqa: E402
from benchlib import E, M, N  # noqa: E402

EVERY, MAX_REPORTS, WARMUP, ROUNDS = 50, 64, 5, 5


def timed_rounds(cases, warmup=WARMUP):
    """cases: [(fn, iters, wall)].  Per case (median ms per call over ROUNDS, spread): device events around the calls, or,
    for a case that synchronises by itself (wall), the host's clock between two device synchronisations.

    The one private timing loop left beside benchlib's two: it synchronises before every block, so that the host's clock
    starts on an idle device, and reads that clock around the same block; benchlib.per_block does neither, and taking both
    in would make it the longer and the less plain of the two."""
    for fn, _, _ in cases:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in cases]
    for r in range(ROUNDS):
        for k, (fn, iters, wall) in enumerate(cases):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ms[k].append((t1 - t0) * 1e3 / iters if wall else e0.elapsed_time(e1) / iters)
    return BL.median_spread(np.array(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--snapshot-iters", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "episode_recorder_c5.json"))
    args = ap.parse_args()
    envs, ags, mons = [], [], []
    for _ in range(4):
        env = BL.c5_env(torch.bfloat16)
        envs.append(env)
        ags.append(BL.warmed(ReworkAgent(epsilon=0.1, record_per_step=4096, min_replay=1000, seed=1, fused_select=True), env))
        mons.append(EpisodeMonitor(env, report_every=EVERY, max_reports=MAX_REPORTS, max_episodes=1))
    cfg = envs[0].cfg
    assert (WARMUP + ROUNDS * args.iters) // EVERY <= MAX_REPORTS
    rec = EpisodeRecorder(envs[1], env_indices=(0,), max_frames=WARMUP + ROUNDS * args.iters)
    rec.begin()

    def step(k):
        mons[k].step(envs[k].reward, ags[k].rollout_step(envs[k]))

    def alone():
        step(0)

    def recorded():
        step(1)
        rec.record()

    def flushed():
        step(2)
        envs[2].flush()

    def snapshotted():
        step(3)
        snapshot_batched(envs[3])

    names = ("step", "step_record", "step_flush", "step_snapshot_batched")
    ts = timed_rounds([(alone, args.iters, False), (recorded, args.iters, False), (flushed, args.iters, False),
                       (snapshotted, args.snapshot_iters, True)])
    c = cfg
    G = c.w * c.h
    read_bytes = E * (N * (24 + 4 + 1 + 1) + G * (4 * c.n_phero + 4 + 1 + 1) + 8 + 4 + 12)  # what snapshot_batched reads per call
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters, snapshot_iters=args.snapshot_iters, rounds=ROUNDS, envs=E,
               ants=N, shape="512 x 512 ants, 256 x 256 cells", format="bfloat16", K=4096, minibatch=264, report_every=EVERY,
               recorded_envs=1, frame_bytes=rec.frame_bytes, static_bytes=rec.static_bytes, snapshot_batched_bytes_read=read_bytes)
    for n, (t, s) in zip(names, ts):
        out[n + "_ms"], out[n + "_spread"] = t, s
    t0 = ts[0][0]
    out.update(record_adds_ms=ts[1][0] - t0, flush_adds_ms=ts[2][0] - t0, snapshot_batched_adds_ms=ts[3][0] - t0,
               snapshot_over_record=(ts[3][0] - t0) / max(ts[1][0] - t0, 1e-9), ant_steps_per_s_recording=M / ts[1][0] * 1e3,
               timing=dict(step="device events", step_record="device events", step_flush="device events",
                           step_snapshot_batched="host clock between device synchronisations"))
    print("  ".join("%s %.4f ms (spread %.1f %%)" % (n, t, 100 * s) for n, (t, s) in zip(names, ts)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
