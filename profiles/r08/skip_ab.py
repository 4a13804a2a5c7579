#!/usr/bin/env python3
"""Same-build A/B of the explored summary: ANTSRL_PERCEIVE_AUTO (summary kept and consumed) against
ANTSRL_PERCEIVE_FAST_NOSKIP (the same fast kernel, summary ignored, no refresh enqueued), on bench.py's workload.

    python profiles/r08/skip_ab.py [--config c3|c2] [--rounds 5] [--age 400] [--steps 200] [--refresh-cost]

One process, ONE handle (one placement of its buffers: the two paths then differ in nothing but the path): per round the
episode is reset, aged and timed once per path, the order alternating.  Prints one line per measurement, ms per step over
`--steps` steps (HIP events around the whole region), and with --refresh-cost the time of one forced refresh
(antsrl_refresh_explored_summary) at ages 64 and `--age` of a fresh episode.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SHAPES = {"c3": dict(E=1024, N=512, W=256, H=256, R=8), "c2": dict(E=256, N=256, W=256, H=256, R=0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--age", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--refresh-cost", action="store_true")
    args = ap.parse_args()
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    s = SHAPES[args.config]
    dev = torch.device("cuda:0")
    cfg = cm.make_cfg(s["E"], s["N"], s["W"], s["H"], n_rocks=s["R"], deposit_strength=256.0, max_time=1 << 30)
    env = BatchedAntsEnv(cfg, dev)
    env.tune_placement()
    init = synth_init(cfg, seed=1234)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    rot = torch.randint(-1, 2, (8, s["E"], s["N"]), generator=g, device=dev, dtype=torch.int8)
    ph = torch.randint(0, 3, (8, s["E"], s["N"]), generator=g, device=dev, dtype=torch.int8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def episode(path, age):
        env.set_perceive_path(path)
        env.reset(init)
        for t in range(age):
            env.step_update(rot[t % 8], ph[t % 8], None)

    def timed(n, t0):
        e0.record()
        for t in range(t0, t0 + n):
            env.step_update(rot[t % 8], ph[t % 8], None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    names = {cm.PERCEIVE_AUTO: "auto  ", cm.PERCEIVE_FAST_NOSKIP: "noskip"}
    for r in range(args.rounds):
        order = (cm.PERCEIVE_FAST_NOSKIP, cm.PERCEIVE_AUTO) if r % 2 == 0 else (cm.PERCEIVE_AUTO, cm.PERCEIVE_FAST_NOSKIP)
        for path in order:
            episode(path, args.age + args.warmup)
            print("%s r%d %s %.5f" % (args.config, r + 1, names[path], timed(args.steps, args.age + args.warmup)), flush=True)
    if args.refresh_cost:
        for age in sorted({64, args.age}):
            # (age - 1 steps: short of the observation behind which the library would refresh by itself)
            episode(cm.PERCEIVE_AUTO, age - 1)
            torch.cuda.synchronize()
            e0.record()
            env.refresh_explored_summary()
            e1.record()
            e1.synchronize()
            first = e0.elapsed_time(e1)
            e0.record()
            env.refresh_explored_summary()
            e1.record()
            e1.synchronize()
            print("%s refresh at age %d: %.4f ms, again right behind it: %.4f ms" % (args.config, age - 1, first, e0.elapsed_time(e1)), flush=True)


if __name__ == "__main__":
    main()
