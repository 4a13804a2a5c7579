#!/usr/bin/env python3
"""Times the training monitor (antsrl_amd.monitor.EpisodeMonitor) at config 5's batch (512 envs x 512 ants,
bfloat16 observations, ReworkAgent, K = 4096 rows recorded per step, minibatch 264, every step trains):

  (a) rollout          ReworkAgent.rollout_step alone (the loop as it was before the monitor)
  (b) + monitor        rollout_step, then EpisodeMonitor.step(env.reward, loss): one launch, a report every 50 steps
  (c) + eager          rollout_step, then the same bookkeeping as eager torch ops with no host read (EagerBook)
  (d) bookkeeping alone: antsrl_monitor_step on a step that does not report and on one that does, with the bytes it moves,
      and EagerBook's two kinds of step

Device events around `--iters` calls per case and round; the cases of a group alternate inside a round; five rounds; the
median over the rounds and their spread, (max - min) / median (profiles/rework_agent_bench.py's method).  One process.

    python profiles/train_driver_bench.py [--iters 100] [--json profiles/train_driver_c5.json]
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
from antsrl_amd.monitor import EpisodeMonitor  # noqa: E402
from benchlib import E, M, N  # noqa: E402

EVERY, MAX_REPORTS, ROUNDS = 50, 64, 5


def rounds(fns, iters):
    """Per fn: (median over ROUNDS of the ms per call, spread of the rounds); the fns alternate inside every round, one
    event pair around `iters` calls of one fn."""
    return BL.median_spread(BL.per_block(fns, iters, rounds=ROUNDS, warmup=5))


class EagerBook:
    """The monitor's bookkeeping written as eager torch ops on device tensors, without a host read: the cast-add, the
    running loss (first loss, then 0.99 * avg + 0.01 * loss) and, on a report step, a reduction per statistic."""

    def __init__(self, device):
        self.er = torch.zeros((E, N), dtype=torch.float64, device=device)
        self.avg = torch.zeros((), dtype=torch.float64, device=device)
        self.n = torch.zeros((), dtype=torch.int64, device=device)
        self.reports = torch.zeros((MAX_REPORTS, E, 3), dtype=torch.float64, device=device)
        self.s = 0

    def step(self, reward, loss, report=None):
        self.er.add_(reward)
        l64 = loss.double()
        self.avg.copy_(torch.where(self.n == 0, l64, 0.99 * self.avg + 0.01 * l64))
        self.n.add_(1)
        self.s += 1
        if (self.s % EVERY == 0) if report is None else report:
            r = self.reports[(self.s // EVERY) % MAX_REPORTS]
            r[:, 0] = self.er.sum(dim=1)
            r[:, 1] = self.er.amin(dim=1)
            r[:, 2] = self.er.amax(dim=1)


def bench_rollout(fmt, iters):
    envs = [BL.c5_env(getattr(torch, fmt)) for _ in range(3)]
    ags = [BL.warmed(ReworkAgent(epsilon=0.1, record_per_step=4096, min_replay=1000, seed=1, fused_select=True), env) for env in envs]
    mon = EpisodeMonitor(envs[1], report_every=EVERY, max_reports=MAX_REPORTS, max_episodes=1)
    book = EagerBook(envs[2].device)
    assert (5 + ROUNDS * iters) // EVERY <= MAX_REPORTS

    def alone():
        ags[0].rollout_step(envs[0])

    def monitored():
        mon.step(envs[1].reward, ags[1].rollout_step(envs[1]))

    def eager():
        book.step(envs[2].reward, ags[2].rollout_step(envs[2]))

    (t0, s0), (t1, s1), (t2, s2) = rounds([alone, monitored, eager], iters)
    print("%-8s rollout_step %.4f ms (spread %.1f %%)  + monitor.step %.4f ms (%.1f %%)  + eager torch %.4f ms (%.1f %%)"
          % (fmt, t0, 100 * s0, t1, 100 * s1, t2, 100 * s2), flush=True)
    return dict(format=fmt, shape="512 x 512 ants, 256 x 256 cells", K=4096, minibatch=264, report_every=EVERY,
                rollout_step_ms=t0, rollout_step_spread=s0, with_monitor_ms=t1, with_monitor_spread=s1,
                with_eager_torch_ms=t2, with_eager_torch_spread=s2, monitor_adds_ms=t1 - t0, eager_adds_ms=t2 - t0,
                ant_steps_per_s_with_monitor=M / t1 * 1e3)


def bench_alone(iters):
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(2)
    reward = torch.randn((E, N), device="cuda", generator=g)
    loss = torch.rand((), device="cuda", generator=g)
    mon = EpisodeMonitor((E, N), report_every=EVERY, max_reports=1, max_episodes=1)
    book = EagerBook(reward.device)

    def native(slot):
        _lib.check(lib.antsrl_monitor_step(_p(mon._state), E, N, 1, 1, _p(reward), _p(loss), 0.0, 1, slot,
                                           _lib.stream(mon.device)), "monitor_step")

    names = ("monitor_step", "monitor_step_report", "eager_torch", "eager_torch_report")
    ts = rounds([lambda: native(-1), lambda: native(0), lambda: book.step(reward, loss, False),
                 lambda: book.step(reward, loss, True)], iters)
    moved = dict(monitor_step=M * (4 + 8 + 8) + 4 + 24, monitor_step_report=M * (4 + 8 + 8) + 4 + 24 + E * 24)
    out = dict(bytes_moved=moved)
    for n, (t, s) in zip(names, ts):
        out[n + "_ms"], out[n + "_spread"] = t, s
        if n in moved:
            out[n + "_gbytes_per_s"] = moved[n] / t * 1e-6
    print("alone: " + ", ".join("%s %.4f ms (spread %.1f %%)" % (n, t, 100 * s) for n, (t, s) in zip(names, ts)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "train_driver_c5.json"))
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters, rounds=ROUNDS, envs=E, ants=N,
               bookkeeping_alone=bench_alone(4 * args.iters), rollout=[bench_rollout("bfloat16", args.iters)])
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
