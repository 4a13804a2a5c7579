#!/usr/bin/env python3
"""Times the linear agent (antsrl_amd.agent.CollectAgent) on the device:

  train      LinearTrainer.step (antsrl_lintrain_step) at B = 264, 4096 and 65 536 against eager torch fp32 running the
             reference's train() arithmetic (agents/collect_agent.py:105-148) with torch.optim.Adam on the same device and
             the same replay arrays, alternating inside one timed loop.
  rollout    CollectAgent.rollout_step at config 5's shape (512 envs x 512 ants, 256 x 256, bfloat16 observations, K = 4096
             rows recorded per step, minibatch 264) with inloop off and on, beside its parts timed alone in the same
             process: the environment step with the in-loop policy (the parent's c5 step) and without it, the standalone
             policy, select, the two record halves, the training step and the in-loop weight refresh.

hipEvents around `--iters` warmed iterations, medians.  Prints one line per case and a JSON summary (--json).

    python profiles/linear_agent_bench.py [--iters 100] [--json profiles/linear_agent_c5.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/linear_agent_bench.py --probe 40   # launches per step
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
from antsrl_amd.train import LinearTrainer  # noqa: E402
from benchlib import E, F, M, N  # noqa: E402

#: what `pytest -s tests/test_gpu_linear_agent.py` printed on an MI355X, and the bounds the tests hold (about 4 x): the
#: kernel against the device-contract restatement (B <= 4096 / B = 65 536), and against the reference's recorded run
TEST_ERRORS = dict(
    contract=dict(gradient_of_tensor_max=dict(measured=[1.99e-7, 6.89e-7], bound=[8e-7, 2.8e-6]),
                  loss_relative=dict(measured=[1.21e-7, 5.01e-7], bound=[5e-7, 2e-6]),
                  heads_in_steps_of_lr=dict(measured=3.73e-5, bound=1e-4), adam_moments="bit for bit"),
    fixture_fp32=dict(loss_relative=dict(measured=[7.66e-5, 7.13e-5, 1.01e-4], bound=4e-4),
                      one_minus_cosine_gradient=dict(measured=2.0e-6, bound=8e-6),
                      one_minus_cosine_delta=dict(measured=4.0e-5, bound=1.6e-4)),
    acting=dict(decisions_left_out=5, decisions=512, cap=0.01))


def timed(fns, iters):
    """Median ms per call of each fn in `fns`, alternating them inside one timed loop."""
    return BL.median(BL.per_call(fns, iters, 10)).tolist()


class EagerRef(torch.nn.Module):
    """CollectModel over ExploreModel in eager torch, and CollectAgent.train's arithmetic around it."""

    def __init__(self, tr):
        super().__init__()
        sd = tr.state_dict()
        self.l1 = torch.nn.Linear(F + 2, 32).cuda()
        self.l2, self.l3, self.t3 = (torch.nn.Linear(32, 3).cuda() for _ in range(3))
        with torch.no_grad():
            for lin, k in ((self.l1, "explore_model.layer1"), (self.l2, "explore_model.layer2"), (self.l3, "layer3"), (self.t3, "layer3")):
                lin.weight.copy_(sd[k + ".weight"])
                lin.bias.copy_(sd[k + ".bias"])
        for p in list(self.l1.parameters()) + list(self.t3.parameters()):
            p.requires_grad = False
        self.opt = torch.optim.Adam([p for p in self.parameters() if p.requires_grad], lr=1e-4)
        self.crit = torch.nn.MSELoss()

    def net(self, x, a, l3):
        out = self.l1(torch.cat([x.view(-1, F), a.view(-1, 2)], dim=1))
        return self.l2(out), l3(out)

    def train_step(self, arrays, idx, discount=0.5):
        st, ast, act, rw, nst, nast, dn = (a[idx] for a in arrays)
        rows = torch.arange(len(rw), device=rw.device)
        with torch.no_grad():
            fr, fp = self.net(nst, nast, self.t3)
            tr_, tp = self.net(st, ast, self.l3)
            tr_[rows, act[:, 0]] = rw + discount * fr.max(dim=1).values * ~dn
            tp[rows, act[:, 1]] = rw + discount * fp.max(dim=1).values * ~dn
        qr, qp = self.net(st, ast, self.l3)
        loss = self.crit(qr, tr_) + self.crit(qp, tp)
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
    tr = LinearTrainer(F, "cuda", seed=1)
    ref = EagerRef(tr)
    l_dev, l_ref = float(tr.step(arrays, idx)), float(ref.train_step(arrays, idx).detach())
    t_dev, t_ref = timed([lambda: tr.step(arrays, idx, keep_grads=False), lambda: ref.train_step(arrays, idx)], iters)
    gathered = 2 * B * (F + 2) * 4
    return dict(B=B, launches=tr.launches(B), step_ms=t_dev, eager_torch_fp32_ms=t_ref, speedup=t_ref / t_dev,
                first_loss=l_dev, first_loss_eager=l_ref, gathered_bytes=gathered, gathered_gbytes_per_s=gathered / t_dev * 1e-6)


def c5_env():
    return BL.c5_env(torch.bfloat16, cm.ACT_CELL_META)


def agent_on(env, inloop, K=4096):
    return BL.warmed(CollectAgent(epsilon=0.1, record_per_step=K, min_replay=1000, seed=1, inloop=inloop), env)


def bench_rollout(iters, K=4096):
    env_a, env_b, env_p = c5_env(), c5_env(), c5_env()
    a, b = agent_on(env_a, False, K), agent_on(env_b, True, K)
    t_off, t_on = timed([lambda: a.rollout_step(env_a), lambda: b.rollout_step(env_b)], iters)
    # the steps that do not train (training=False: act, record, step): the in-loop actions are taken there
    t_off_nt, t_on_nt = timed([lambda: a.rollout_step(env_a, False), lambda: b.rollout_step(env_b, False)], iters)
    hits = b.inloop_hits
    # ---- the parts, alone (env_p: a third environment; b's handle has the in-loop policy)
    p = agent_on(env_p, False, K)
    rot, ph = (t.clone() for t in p.get_action(env_p.obs, env_p.agent_state, False, env=env_p))
    rm, kw = p.replay_memory, p._record_kw()
    idx = torch.randint(0, len(rm), (264,), device="cuda")

    def rec():
        rm.record_pre(env_p.obs, env_p.agent_state, None, rot.view(-1), ph.view(-1), **kw)
        rm.record_post(env_p.obs, env_p.agent_state, None, env_p.reward.view(-1), env_p.done)

    names = ("env_step_inloop_policy", "env_step_plain", "policy_standalone", "select", "record_pre_post", "train_step",
             "inloop_refresh")
    ts = timed([lambda: env_b.step_update(env_b.next_rotation, env_b.next_pheromone),
                lambda: env_p.step_update(rot.view(E, N), ph.view(E, N)),
                lambda: p.policy.act(env_p.obs, env_p.agent_state, env=env_p),
                lambda: p.get_action(env_p.obs, env_p.agent_state, True, env=env_p),  # act + select: select = this - act
                rec, lambda: p.trainer.step(rm, idx, keep_grads=False), b.refresh_inloop], iters)
    parts = dict(zip(names, ts))
    parts["select"] = max(parts["select"] - parts["policy_standalone"], 0.0)
    sum_off = parts["env_step_plain"] + parts["policy_standalone"] + parts["select"] + parts["record_pre_post"] + parts["train_step"]
    return dict(shape="512 x 512 ants, 256 x 256, bf16 observations", K=K, minibatch=264, rollout_step_ms=t_off,
                rollout_step_inloop_ms=t_on, rollout_step_not_training_ms=t_off_nt, rollout_step_not_training_inloop_ms=t_on_nt,
                inloop_hits_not_training=hits, ant_steps_per_s=M / t_off * 1e3, parts_ms=parts, sum_of_parts_ms=sum_off,
                gap_ms=t_off - sum_off, inloop_hits_total=b.inloop_hits)


def probe(steps):
    env = c5_env()
    ag = agent_on(env, False)
    for _ in range(steps):
        ag.rollout_step(env)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "linear_agent_c5.json"))
    ap.add_argument("--probe", type=int, default=0, help="run this many rollout_steps and exit (under rocprofv3)")
    ap.add_argument("--skip-rollout", action="store_true")
    args = ap.parse_args()
    if args.probe:
        return probe(args.probe)
    out = dict(device=torch.cuda.get_device_name(0), iters=args.iters, test_errors=TEST_ERRORS, train=[])
    for B in (264, 4096, 65536):
        r = bench_train(B, args.iters)
        out["train"].append(r)
        print("train B = %6d: %d launch(es) %.4f ms, eager torch fp32 %.4f ms (x %.1f), %.1f GB/s gathered"
              % (B, r["launches"], r["step_ms"], r["eager_torch_fp32_ms"], r["speedup"], r["gathered_gbytes_per_s"]), flush=True)
    if not args.skip_rollout:
        r = bench_rollout(max(20, args.iters // 2))
        out["rollout"] = r
        print("not training: rollout_step %.3f ms, inloop %.3f ms (%d in-loop hits)" % (r["rollout_step_not_training_ms"], r["rollout_step_not_training_inloop_ms"], r["inloop_hits_not_training"]))
        print("rollout_step %.3f ms (inloop %.3f ms), sum of parts %.3f ms, gap %.3f ms; parts: %s"
              % (r["rollout_step_ms"], r["rollout_step_inloop_ms"], r["sum_of_parts_ms"], r["gap_ms"],
                 ", ".join("%s %.3f" % kv for kv in r["parts_ms"].items())), flush=True)
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
