#!/usr/bin/env python3
"""Times the explore agent (antsrl_amd.agent.ExploreAgent) on the device:

  train      ExploreTrainer.step (antsrl_exptrain_step) at B = 256 and 4096, F = 294, against eager torch fp32 running the
             same arithmetic (ExploreModel with CollectModel.forward's concat, ExploreAgentPytorch.train) with
             torch.optim.Adam on the same device and the same replay arrays, alternating inside one timed loop.
  rollout    ExploreAgent.rollout_step at config 5's shape (512 envs x 512 ants, 256 x 256, bfloat16 observations, K = 4096
             rows recorded per step, minibatch 256) with inloop off and on, beside its parts timed alone in the same
             process.

The method is profiles/linear_agent_bench.py's: hipEvents around `--iters` warmed iterations, medians.

    python profiles/explore_agent_bench.py [--iters 100] [--json profiles/explore_agent_c5.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/explore_agent_bench.py --probe 40   # launches per step
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.agent import ExploreAgent  # noqa: E402
from antsrl_amd.train import ExploreTrainer  # noqa: E402
from benchlib import E, F, M, N  # noqa: E402


def timed(fns, iters):
    """Median ms per call of each fn in `fns`, alternating them inside one timed loop."""
    return BL.median(BL.per_call(fns, iters, 10)).tolist()


def c5_env():
    return BL.c5_env(torch.bfloat16, cm.ACT_CELL_META)


class EagerRef(torch.nn.Module):
    """ExploreModel in eager torch, and ExploreAgentPytorch.train's arithmetic around it."""

    def __init__(self, tr):
        super().__init__()
        sd = tr.state_dict()
        self.l1, self.t1 = (torch.nn.Linear(F + 2, 32).cuda() for _ in range(2))
        self.l2, self.t2 = (torch.nn.Linear(32, 3).cuda() for _ in range(2))
        with torch.no_grad():
            for lin, k in ((self.l1, "layer1"), (self.t1, "layer1"), (self.l2, "layer2"), (self.t2, "layer2")):
                lin.weight.copy_(sd[k + ".weight"])
                lin.bias.copy_(sd[k + ".bias"])
        for p in list(self.t1.parameters()) + list(self.t2.parameters()):
            p.requires_grad = False
        self.opt = torch.optim.Adam([p for p in self.parameters() if p.requires_grad], lr=1e-4)
        self.crit = torch.nn.MSELoss()

    def train_step(self, arrays, idx, discount=0.5):
        st, ast, act, rw, nst, nast, dn = (a[idx] for a in arrays)
        rows = torch.arange(len(rw), device=rw.device)
        net = lambda l1, l2, x, a: l2(l1(torch.cat([x.view(-1, F), a.view(-1, 2)], dim=1)))  # noqa: E731
        with torch.no_grad():
            new_qs = rw + discount * net(self.t1, self.t2, nst, nast).max(dim=1).values * ~dn
            target_qs = net(self.l1, self.l2, st, ast)
            target_qs[rows, act[:, 0]] = new_qs
        loss = self.crit(net(self.l1, self.l2, st, ast), target_qs)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss


def bench_train(B, iters):
    rows = max(50000, 2 * B)
    g = torch.Generator(device="cuda").manual_seed(B)
    d = dict(device="cuda", generator=g)
    arrays = (torch.rand((rows, F), **d), torch.rand((rows, 2), **d), torch.randint(0, 3, (rows, 2), **d), torch.randn((rows,), **d),
              torch.rand((rows, F), **d), torch.rand((rows, 2), **d), torch.rand((rows,), **d) < 0.1)
    idx = torch.randint(0, rows, (B,), **d)
    tr = ExploreTrainer(F, "cuda", seed=1)
    ref = EagerRef(tr)
    l_dev, l_ref = float(tr.step(arrays, idx)), float(ref.train_step(arrays, idx).detach())
    t_dev, t_ref = timed([lambda: tr.step(arrays, idx, keep_grads=False), lambda: ref.train_step(arrays, idx)], iters)
    return dict(B=B, trained_floats=tr.trained_floats, launches=tr.launches(B), step_ms=t_dev, eager_torch_fp32_ms=t_ref,
                speedup=t_ref / t_dev, first_loss=l_dev, first_loss_eager=l_ref)


def agent_on(env, inloop, K=4096):
    return BL.warmed(ExploreAgent(epsilon=0.1, record_per_step=K, min_replay=1000, seed=1, inloop=inloop), env)


def bench_rollout(iters, K=4096):
    env_a, env_b, env_p = c5_env(), c5_env(), c5_env()
    a, b = agent_on(env_a, False, K), agent_on(env_b, True, K)
    h0 = b.inloop_hits
    t_off, t_on = timed([lambda: a.rollout_step(env_a), lambda: b.rollout_step(env_b)], iters)
    hits, steps = b.inloop_hits - h0, iters + 10
    p = agent_on(env_p, False, K)
    rot = p.get_action(env_p.obs, env_p.agent_state, False, env=env_p)[0].clone()
    rm, kw = p.replay_memory, p._record_kw()
    idx = torch.randint(0, len(rm), (256,), device="cuda")

    def rec():
        rm.record_pre(env_p.obs, env_p.agent_state, None, rot.view(-1), None, **kw)
        rm.record_post(env_p.obs, env_p.agent_state, None, env_p.reward.view(-1), env_p.done)

    names = ("env_step_inloop_policy", "env_step_plain", "policy_standalone", "select", "record_pre_post", "train_step",
             "inloop_refresh", "sync_target")
    ts = timed([lambda: env_b.step_update(env_b.next_rotation, None),
                lambda: env_p.step_update(rot.view(E, N), None),
                lambda: p.policy.act(env_p.obs, env_p.agent_state, env=env_p),
                lambda: p.get_action(env_p.obs, env_p.agent_state, True, env=env_p),  # act + select: select = this - act
                rec, lambda: p.trainer.step(rm, idx, keep_grads=False), b.refresh_inloop, p.trainer.sync_target], iters)
    parts = dict(zip(names, ts))
    parts["select"] = max(parts["select"] - parts["policy_standalone"], 0.0)
    sum_off = parts["env_step_plain"] + parts["policy_standalone"] + parts["select"] + parts["record_pre_post"] + parts["train_step"]
    return dict(shape="512 x 512 ants, 256 x 256, bf16 observations", K=K, minibatch=256, rollout_step_ms=t_off,
                rollout_step_inloop_ms=t_on, inloop_hits=hits, inloop_steps=steps, ant_steps_per_s=M / t_off * 1e3,
                ant_steps_per_s_inloop=M / t_on * 1e3, parts_ms=parts, sum_of_parts_ms=sum_off, gap_ms=t_off - sum_off)


def probe(steps):
    env = c5_env()
    ag = agent_on(env, False)
    for _ in range(steps):
        ag.rollout_step(env)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "explore_agent_c5.json"))
    ap.add_argument("--probe", type=int, default=0, help="run this many rollout_steps and exit (under rocprofv3)")
    ap.add_argument("--skip-rollout", action="store_true")
    args = ap.parse_args()
    if args.probe:
        return probe(args.probe)
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters, train=[])
    for B in (256, 4096):
        r = bench_train(B, args.iters)
        out["train"].append(r)
        print("train B = %6d: %d launches %.4f ms, eager torch fp32 %.4f ms (x %.1f)"
              % (B, r["launches"], r["step_ms"], r["eager_torch_fp32_ms"], r["speedup"]), flush=True)
    if not args.skip_rollout:
        r = bench_rollout(max(20, args.iters // 2))
        out["rollout"] = r
        print("rollout_step %.3f ms (inloop %.3f ms, %d hits in %d steps), sum of parts %.3f ms, gap %.3f ms; parts: %s"
              % (r["rollout_step_ms"], r["rollout_step_inloop_ms"], r["inloop_hits"], r["inloop_steps"], r["sum_of_parts_ms"],
                 r["gap_ms"], ", ".join("%s %.3f" % kv for kv in r["parts_ms"].items())), flush=True)
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
