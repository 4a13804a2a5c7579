#!/usr/bin/env python3
"""Times the joint training step and CollectAgent(train_layer1=True) on the device:

  train      JointTrainer.step (antsrl_jointtrain_step) at B = 264 and 4096, F = 294, alternating inside one timed loop
             against eager torch fp32 running the same arithmetic (CollectModel over ExploreModel with layer1 trainable,
             CollectAgent.train, torch.optim.Adam over all six tensors) on the same replay arrays, and against
             LinearTrainer.step, the frozen step.
  rollout    CollectAgent(train_layer1=True).rollout_step at config 5's shape (512 envs x 512 ants, 256 x 256, bfloat16
             observations, K = 4096 rows recorded per step, minibatch 264) against CollectAgent() in the same process.

The method is profiles/explore_agent_bench.py's: device events around warmed iterations that alternate the candidates in
one process, medians; the spread of each (10th and 90th percentile) is reported beside it.

    python profiles/joint_agent_bench.py [--iters 60] [--json profiles/joint_agent_c5.json]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.agent import CollectAgent  # noqa: E402
from antsrl_amd.train import JointTrainer, LinearTrainer  # noqa: E402
from benchlib import F, M  # noqa: E402
from linear_agent_bench import EagerRef as FrozenEagerRef  # noqa: E402  (a model, not harness: the one import between benches)


def timed(fns, iters):
    """Per fn in `fns`, [median, 10th percentile, 90th percentile] ms per call, alternating them inside one timed loop."""
    return BL.p50_p10_p90(BL.per_call(fns, iters, 10)).tolist()


def c5_env():
    return BL.c5_env(torch.bfloat16, cm.ACT_CELL_META)


class EagerRef(FrozenEagerRef):
    """linear_agent_bench.EagerRef with the freeze of layer1 lifted: Adam over all six tensors."""

    def __init__(self, tr):
        super().__init__(tr)
        for p in self.l1.parameters():
            p.requires_grad = True
        self.opt = torch.optim.Adam([p for p in self.parameters() if p.requires_grad], lr=1e-4)


def bench_train(B, iters):
    rows = max(50000, 2 * B)
    g = torch.Generator(device="cuda").manual_seed(B)
    d = dict(device="cuda", generator=g)
    arrays = (torch.rand((rows, F), **d), torch.rand((rows, 2), **d), torch.randint(0, 3, (rows, 2), **d), torch.randn((rows,), **d),
              torch.rand((rows, F), **d), torch.rand((rows, 2), **d), torch.rand((rows,), **d) < 0.1)
    idx = torch.randint(0, rows, (B,), **d)
    tr, frozen = JointTrainer(F, "cuda", seed=1), LinearTrainer(F, "cuda", seed=1)
    ref = EagerRef(tr)
    l_dev, l_ref = float(tr.step(arrays, idx)), float(ref.train_step(arrays, idx).detach())
    t = timed([lambda: tr.step(arrays, idx, keep_grads=False), lambda: ref.train_step(arrays, idx),
               lambda: frozen.step(arrays, idx, keep_grads=False)], iters)
    (t_dev, *s_dev), (t_ref, *s_ref), (t_frz, *s_frz) = t
    return dict(B=B, trained_floats=tr.trained_floats, launches=tr.launches(B), step_ms=t_dev, step_p10_p90_ms=s_dev,
                eager_torch_fp32_ms=t_ref, eager_p10_p90_ms=s_ref, speedup=t_ref / t_dev, frozen_step_ms=t_frz,
                frozen_p10_p90_ms=s_frz, frozen_launches=frozen.launches(B), over_frozen_ms=t_dev - t_frz,
                first_loss=l_dev, first_loss_eager=l_ref)


def agent_on(env, train_layer1, K=4096):
    return BL.warmed(CollectAgent(epsilon=0.1, record_per_step=K, min_replay=1000, seed=1, train_layer1=train_layer1), env)


def bench_rollout(iters, K=4096):
    env_a, env_b = c5_env(), c5_env()
    a, b = agent_on(env_a, False, K), agent_on(env_b, True, K)
    (t_frz, *s_frz), (t_joint, *s_joint) = timed([lambda: a.rollout_step(env_a), lambda: b.rollout_step(env_b)], iters)
    return dict(shape="512 x 512 ants, 256 x 256, bf16 observations", K=K, minibatch=264, rollout_step_ms=t_joint,
                rollout_p10_p90_ms=s_joint, frozen_rollout_step_ms=t_frz, frozen_p10_p90_ms=s_frz, ratio=t_joint / t_frz,
                ant_steps_per_s=M / t_joint * 1e3, frozen_ant_steps_per_s=M / t_frz * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "joint_agent_c5.json"))
    ap.add_argument("--skip-rollout", action="store_true")
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters, train=[])
    for B in (264, 4096):
        r = bench_train(B, args.iters)
        out["train"].append(r)
        print("train B = %6d: %d launches %.4f ms, eager torch fp32 %.4f ms (x %.1f), frozen step %.4f ms (+ %.4f ms)"
              % (B, r["launches"], r["step_ms"], r["eager_torch_fp32_ms"], r["speedup"], r["frozen_step_ms"], r["over_frozen_ms"]),
              flush=True)
    if not args.skip_rollout:
        r = bench_rollout(args.iters)
        out["rollout"] = r
        print("rollout_step %.3f ms, frozen %.3f ms (x %.3f)" % (r["rollout_step_ms"], r["frozen_rollout_step_ms"], r["ratio"]),
              flush=True)
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
