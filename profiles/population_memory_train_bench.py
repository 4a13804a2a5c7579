#!/usr/bin/env python3
"""Times the training step of a population of memory nets (antsrl_amd.population.PopulationMemoryTrainer) at
the workload's shape: F = 294, power 5, mem 20, B = 264, a synthetic ring of 4096 rows per member.

  single        MemoryTrainer.step alone (16 + 1 launches)
  entries       the same step as the bare calls of its two entries (antsrl_memtrain_grad, antsrl_memtrain_apply) on
                pointers taken once: what MemoryTrainer.step costs on the host beyond them shows against `single`
  population    PopulationMemoryTrainer.step at P = 1, 4, 16 and 64 (--members): 17 launches whatever P is
  sequential    at P = 4 and 16 (--sequential), P MemoryTrainers stepped one after another with the single entries on
                the same slabs and rows (17 P launches): the only way there was before, and the yardstick

Every configuration is built and warmed first.  A figure is the time between two device events around `--steps` (>= 200)
consecutive steps, divided by the steps; it is taken `--repeats` times, the configurations alternated inside a repeat, and
reported as the median of the repeats with their spread (max - min), in µs per step and per member-step.  The bar
(DESIGN §10): a difference is called only if it exceeds three times the yardstick's own spread.  Prints one line per
configuration and one JSON line.  Without a GPU it exits with an error.

    python profiles/population_memory_train_bench.py [--steps 200] [--repeats 3] [--members 1,4,16,64] [--sequential 4,16]
                                                     [--json profiles/population_memory_train.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from benchlib import F  # noqa: E402

POWER, MEM, B, ROWS = 5, 20, 264, 4096


def members(P):
    return BL.members(P, 1e-5, epsilon=None)


def synthetic_ring(P, seed):
    """A full ring of ROWS rows per member: observations 30 % nonzero, agent states and memory in (-1, 1), normal rewards."""
    from antsrl_amd.population import PopulationReplayMemory
    g = torch.Generator(device="cuda").manual_seed(seed)
    ring = PopulationReplayMemory(P, ROWS, (7, 7, 6), device="cuda", agent_states_space=(2 + MEM,))
    r = lambda t: torch.rand(t.shape, generator=g, device="cuda")  # noqa: E731
    for t in (ring.states, ring.new_states):
        t.copy_((r(t) < 0.3).float() * r(t))
    for t in (ring.agent_states, ring.new_agent_states):
        t.copy_(r(t) * 2 - 1)
    ring.actions.copy_(torch.randint(0, 3, ring.actions.shape, generator=g, device="cuda"))
    ring.rewards.copy_(torch.randn(ring.rewards.shape, generator=g, device="cuda"))
    ring.dones.copy_(r(ring.dones) < 0.2)
    ring.fill = ROWS
    return ring


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", default="1,4,16,64", help="the population sizes to time")
    ap.add_argument("--sequential", default="4,16", help="of those, the sizes to time one member after another as well")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "population_memory_train.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("population_memory_train_bench.py: no GPU: the step is HIP for gfx950 and has no other form")
    assert args.steps >= 200, "a figure is taken over at least 200 steps"
    from bench import device_identity
    import ctypes as C
    from antsrl_amd import _lib, population
    from antsrl_amd.train import MemoryTrainer
    sizes, seq_sizes = ([int(x) for x in v.split(",") if x] for v in (args.members, args.sequential))
    assert set(seq_sizes) <= set(sizes), "--sequential names sizes that --members does not"

    configs = []  # (kind, P, launches per step, fn)
    one_ring = synthetic_ring(1, 1)
    one = MemoryTrainer(F, "cuda", discount=0.5, lr=1e-5, power=POWER, mem_size=MEM, seed=1)
    one_arrays = tuple(getattr(one_ring, n)[0] for n in population.RING_NAMES)
    one_idx = torch.randint(0, ROWS, (B,), device="cuda")
    configs.append(("single", 1, 17, lambda: one.step(one_arrays, one_idx)))
    raw = MemoryTrainer(F, "cuda", discount=0.5, lr=1e-5, power=POWER, mem_size=MEM, seed=1)
    raw.step(one_arrays, one_idx)  # sizes the workspace
    lib, st, shape, raw_loss = _lib.load(), _lib.stream(raw.device), C.byref(raw.shape), torch.zeros((), device="cuda")
    grad_args = [_lib.ptr(t) for t in (raw._model, raw._target) + one_arrays + (one_idx,)]
    grad_tail = [_lib.ptr(t) for t in (raw.grads, raw_loss, raw._work)]

    def entries():
        raw.step_count += 1
        _lib.check(lib.antsrl_memtrain_grad(shape, *grad_args, B, raw.discount, *grad_tail, st), "memtrain_grad")
        _lib.check(lib.antsrl_memtrain_apply(shape, grad_args[0], grad_tail[0], raw.step_count, raw.lr, raw.betas[0], raw.betas[1],
                                             raw.eps, st), "memtrain_apply")
    configs.append(("entries", 1, 17, entries))
    rings = {}
    for P in sizes:
        m = members(P)
        g = population._Geometry(P, P, 8, 0, F, torch.float32)  # the training entry reads the spec's members and n_features only
        tr = population.PopulationMemoryTrainer(g, "cuda:0", [x["seed"] for x in m], [x["discount"] for x in m],
                                                [x["learning_rate"] for x in m], power=POWER, mem_size=MEM)
        rings[P] = (synthetic_ring(P, 2 + P), torch.randint(0, ROWS, (P, B), device="cuda"))
        ring, idx = rings[P]
        spec = tr._spec()
        assert tr._sizes(B)[4] == 17
        configs.append(("population", P, 17, lambda tr=tr, ring=ring, idx=idx, spec=spec: tr.step(ring, idx, spec)))
    for P in seq_sizes:
        ring, idx = rings[P]
        trs = [MemoryTrainer(F, "cuda", discount=x["discount"], lr=x["learning_rate"], power=POWER, mem_size=MEM, seed=x["seed"])
               for x in members(P)]
        slabs = [tuple(getattr(ring, n)[p] for n in population.RING_NAMES) for p in range(P)]

        def seq(trs=trs, slabs=slabs, idx=idx):
            for p, t in enumerate(trs):
                t.step(slabs[p], idx[p])
        configs.append(("sequential", P, 17 * P, seq))

    # the warm-up of every shape (the workspaces, the code objects, the clocks), then per repeat and configuration two
    # device events around `steps` consecutive steps and a synchronise: us [configuration][repeat]
    times = BL.per_block([fn for _, _, _, fn in configs], args.steps, rounds=args.repeats, warmup=10, sync_blocks=True) * 1000.0
    med, spread = BL.median(times), BL.abs_spread(times)

    out = dict(device=device_identity(torch, torch.cuda.current_device()), steps=args.steps, repeats=args.repeats,
               shape="F = %d, power %d, mem %d, B = %d, ring %d rows per member" % (F, POWER, MEM, B, ROWS),
               figures="us_per_step: median over the repeats of (device time of `steps` consecutive steps) / steps; spread_us: "
                       "max - min over the repeats; us_per_member_step: us_per_step / P", results=[])
    for (kind, P, launches, _), m, s in zip(configs, med, spread):
        r = dict(kind=kind, P=P, launches=launches, us_per_step=float(m), spread_us=float(s), us_per_member_step=float(m / P),
                 spread_us_per_member_step=float(s / P))
        out["results"].append(r)
        print("%-10s P = %2d (%4d launches): %10.1f us per step (spread %.1f), %9.1f us per member-step" % (kind, P, launches, m, s, m / P),
              flush=True)
    find = lambda kind, P: next((r for r in out["results"] if r["kind"] == kind and r["P"] == P), None)  # noqa: E731
    single = find("single", 1)
    claims = {}
    if find("population", 1):
        d = find("population", 1)["us_per_step"] - single["us_per_step"]
        claims["P1_minus_single_us"] = d
        claims["P1_unchanged_within_three_spreads_of_single"] = bool(abs(d) <= 3.0 * single["spread_us"])
    for P in seq_sizes:
        pop, seq = find("population", P), find("sequential", P)
        claims["P%d_population_to_sequential" % P] = pop["us_per_step"] / seq["us_per_step"]
        claims["P%d_below_sequential_by_three_spreads" % P] = bool(pop["us_per_step"] < seq["us_per_step"] - 3.0 * seq["spread_us"])
    claims["entries_minus_single_us"] = find("entries", 1)["us_per_step"] - single["us_per_step"]
    if find("population", 1):
        claims["P1_minus_entries_us"] = find("population", 1)["us_per_step"] - find("entries", 1)["us_per_step"]
    out["claims"] = claims
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
