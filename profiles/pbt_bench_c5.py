#!/usr/bin/env python3
"""Times population-based training's device side (antsrl_amd/pbt.py) at config 5's batch: 512 environments
x 512 ants on 256 x 256 cells, bfloat16 observations, a rework and a memory population of P = 16 members (32 environments
each), K = 4096 rows recorded per member and step, B = 264, the default ring of 50000 rows per member (a `states` slab is
58.8 MB).

  fitness      antsrl_pop_fitness alone on the monitor's episode_reward (512 x 512 float64)
  exploit      _Population.exploit of 1 and of 4 pairs, with and without the ring, beside
                 torch_loop   the same pairs as copy_member made them before there was an exploit, stated here: per
                              tensor and pair select(dim, dst).copy_(select(dim, src)), and for the memory population the
                              rows of both memory halves
                 bench_copy   antsrl_bench_copy (the library's plain 16-byte copy) of the same number of bytes
  generation   one generation as driver.train_population makes it: record, the read of the row, pbt_plan and the
               exploit of its pairs, on the host's clock to the end of the exploit on the device; beside a 2000-step
               episode's rollout_steps at the step time of profiles/population_rework_c5.json (P = 16)

A device figure is the median of `--iters` calls, one event pair per call (so a call whose enqueue takes the host longer
than the device takes to run it shows the host's time); every figure is taken `--repeats` times and reported as the median
of the repeats with their spread (max - min), in µs.  The bar for copy_member: one pair through the entry is
not slower than the torch loop by more than the torch loop's own spread.  Prints one line per figure and one JSON line.

    python profiles/pbt_bench_c5.py [--iters 20] [--repeats 3] [--json profiles/pbt_c5.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from benchlib import E, N  # noqa: E402

P, K, B, MIN_REPLAY = 16, 4096, 264, 1000
PAIRS = {1: ([0], [8]), 4: ([0, 0, 1, 2], [8, 9, 10, 11])}


def figure(fns, iters, repeats):
    """[(median over the repeats of the median of `iters` calls, max - min over the repeats)] per fn, in µs; the fns are
    interleaved inside an iteration."""
    a = np.array([BL.median(BL.per_call(fns, iters, 3)) for _ in range(repeats)]).T * 1000.0  # [fn, repeat]
    return list(zip(BL.median(a).tolist(), BL.abs_spread(a).tolist()))


def torch_loop(pop, src, dst, ring):
    """The exploit as a torch copy per tensor and pair."""
    from antsrl_amd.replay import ring_arrays
    tensors = list(pop._member_tensors())  # (the memory population's lists both memory halves as [P][Mm][mem])
    if ring:
        tensors += [(a, 0) for a in ring_arrays(pop.replay_memory)]
    for s, d in zip(src, dst):
        for t, dim in tensors:
            t.select(dim, d).copy_(t.select(dim, s))


def bench_population(name, pop, env, iters, repeats):
    from antsrl_amd import _lib
    lib, st = _lib.load(), _lib.stream(env.device)
    out = dict(population=name, P=P, exploit=[])
    for n_pairs, (src, dst) in PAIRS.items():
        for ring in (False, True):
            nbytes = n_pairs * sum(b for _, b in pop._member_arrays(ring))
            copied = (nbytes + 15) // 16 * 16  # (the plain copy moves whole 16-byte units)
            a, b = (torch.empty((copied,), dtype=torch.uint8, device=env.device) for _ in range(2))
            (e, es), (t, ts), (c, cs) = figure([lambda: pop.exploit(src, dst, ring), lambda: torch_loop(pop, src, dst, ring),
                                                lambda: _lib.check(lib.antsrl_bench_copy(_lib.ptr(b), _lib.ptr(a), copied, st))],
                                               iters, repeats)
            del a, b
            r = dict(pairs=n_pairs, ring=ring, arrays=len(pop._member_arrays(ring)), bytes=nbytes, exploit_us=e, exploit_spread_us=es,
                     torch_loop_us=t, torch_loop_spread_us=ts, bench_copy_us=c, bench_copy_spread_us=cs,
                     not_slower_than_loop_by_its_spread=bool(e <= t + ts))
            out["exploit"].append(r)
            print("%-7s %d pair(s), ring %-5s %2d arrays, %11d bytes: exploit %8.1f (spread %.1f)  torch loop %8.1f (spread %.1f)  "
                  "bench_copy %8.1f (spread %.1f) us" % (name, n_pairs, ring, r["arrays"], nbytes, e, es, t, ts, c, cs), flush=True)
    return out


def bench_generation(pop, env, mon, repeats, rounds=10):
    """Host clock, µs: record, the read, the plan, the exploit, to the end of the exploit on the device."""
    from antsrl_amd.pbt import PopulationFitness, pbt_plan
    fit = PopulationFitness(pop, max_rows=1)
    tr = pop.trainer
    parts = np.zeros((repeats, rounds, 4))
    n_pairs = 0
    for r in range(repeats):
        for i in range(rounds + 1):  # (the first round warms up)
            rng = np.random.default_rng(i)
            fit.n_rows = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = fit.record(mon)
            row = fit.row(g)
            t1 = time.perf_counter()
            src_of, lr, discount = pbt_plan(row[:, 0], tr.lr, tr.discount, quantile=0.25, lr_bounds=(1e-6, 1e-2), gap_bounds=(1e-3, 0.5),
                                            rng=rng)
            dst = np.nonzero(src_of != np.arange(P))[0]
            t2 = time.perf_counter()
            pop.exploit(src_of[dst], dst, True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            n_pairs = len(dst)
            if i:
                parts[r, i - 1] = (t1 - t0, t2 - t1, t3 - t2, t3 - t0)
    med = np.median(parts, axis=1) * 1e6  # [repeat, part]
    names = ("record_and_read_us", "plan_us", "exploit_us", "generation_us")
    return dict(pairs=n_pairs, **{n: float(np.median(med[:, k])) for k, n in enumerate(names)},
                **{n.replace("_us", "_spread_us"): float(med[:, k].max() - med[:, k].min()) for k, n in enumerate(names)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "pbt_c5.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pbt_bench_c5.py: no GPU: the entries are HIP for gfx950 and have no other form")
    from bench import device_identity
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.monitor import EpisodeMonitor
    from antsrl_amd.population import PopulationMemoryAgent, PopulationReworkAgent
    lib = _lib.load()
    env = BL.c5_env(torch.bfloat16, cm.ACT_CELL_META)
    st = _lib.stream(env.device)
    out = dict(device=device_identity(torch, torch.cuda.current_device()), iters=args.iters, repeats=args.repeats,
               shape="%d x %d ants, 256 x 256, bf16 observations, P = %d, K = %d per member, B = %d, ring 50000 rows per member"
                     % (E, N, P, K, B),
               figures="us: median over the repeats of the median of `iters` calls (one event pair per call); spread_us: max - min "
                       "over the repeats; generation: the host's clock")

    # the fitness alone, on rewards of every sign
    mon = EpisodeMonitor(env, report_every=50, max_reports=1, max_episodes=1)
    mon.episode_reward.normal_()
    row = torch.zeros((P, 3), dtype=torch.float64, device=env.device)
    (f, fs), = figure([lambda: _lib.check(lib.antsrl_pop_fitness(_lib.ptr(mon.episode_reward), E, N, P, _lib.ptr(row), st))],
                      args.iters, args.repeats)
    out["fitness"] = dict(us=f, spread_us=fs, bytes_read=E * N * 8)
    print("antsrl_pop_fitness, %d x %d float64, P = %d: %.1f us (spread %.1f)" % (E, N, P, f, fs), flush=True)

    out["populations"] = []
    kw = dict(record_per_step=K, minibatch=B, min_replay=MIN_REPLAY, seed=1)
    for name, make in (("rework", lambda: PopulationReworkAgent(BL.members(P, 1e-4), **kw)),
                       ("memory", lambda: PopulationMemoryAgent(BL.members(P, 1e-5), mem_size=20, power=5, **kw))):
        pop = BL.warmed(make(), env)
        r = bench_population(name, pop, env, args.iters, args.repeats)
        if name == "rework":
            g = bench_generation(pop, env, mon, args.repeats)
            step_ms = next(x for x in json.load(open(os.path.join(ROOT, "profiles", "population_rework_c5.json")))["population"]
                           if x["P"] == P)["ms"]["rollout_step"]
            g.update(rollout_step_ms=step_ms, episode_of_2000_steps_ms=2000 * step_ms,
                     share_of_the_episode=g["generation_us"] / (2000.0 * step_ms * 1000.0))
            out["generation"] = g
            print("generation (%d pairs, ring): record + read %.1f, plan %.1f, exploit %.1f, in all %.1f us (spread %.1f) = %.5f of a "
                  "2000-step episode (%.1f ms)" % (g["pairs"], g["record_and_read_us"], g["plan_us"], g["exploit_us"], g["generation_us"],
                                                   g["generation_spread_us"], g["share_of_the_episode"], g["episode_of_2000_steps_ms"]), flush=True)
        out["populations"].append(r)
        del pop
        torch.cuda.empty_cache()
    one = [x for r in out["populations"] for x in r["exploit"] if x["pairs"] == 1]
    out["copy_member_bar"] = dict(rule="one pair through the entry is not slower than the torch loop by more than the loop's own spread",
                                  holds=bool(all(x["not_slower_than_loop_by_its_spread"] for x in one)))
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
