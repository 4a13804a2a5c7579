#!/usr/bin/env python3
"""Times the rework agent's training step (ReworkTrainer.step and .grad: antsrl_reworktrain_*) at F = 294 (7 x 7 x 6) on
B = 264 (the reference's minibatch) and B = 4096 rows drawn from a replay of 50 000, against, on the same inputs, in the
same process and alternating round by round, eager torch fp32 on the device doing the body of the reference's train():
both forwards under no_grad, the two index assignments, the two MSELosses, backward and torch.optim.Adam over the 20
tensors: what a user has without these kernels.  Every figure is the median over the rounds of a mean over enough steps
to fill a good fraction of a second, between device events.  Prints one line per B and a JSON summary.

    python profiles/rework_train_bench.py [--rounds 5] [--json out.json]

The step's four launches are timed by the profiler in a run of its own, which this script only feeds:

    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/rework_train_bench.py --loop 2000 --B 264
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import benchlib as BL  # noqa: E402

from antsrl_amd.train import ReworkTrainer  # noqa: E402


class Eager:
    """The reference's model, target model, criterion and optimizer as eager torch on the device."""

    def __init__(self, sd, discount=0.5, lr=1e-4):
        self.p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        self.t = {k: v.clone() for k, v in sd.items()}
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr)
        self.discount = discount

    @staticmethod
    def net(W, st, ast):
        x = torch.cat([st, ast], dim=1)
        L = lambda n, t: Fn.linear(t, W[n + ".weight"], W[n + ".bias"])  # noqa: E731
        g = L("layer4", L("layer3", L("layer2", L("layer1", x))))
        return (L("rotation_layer4", L("rotation_layer3", L("rotation_layer2", L("rotation_layer1", g)))),
                L("pheromone_layer2", L("pheromone_layer1", g)))

    def step(self, arrays, idx):
        st, ast, act, rw, nst, nast, dn = (a[idx] for a in arrays)
        rows = torch.arange(len(idx), device=idx.device)
        with torch.no_grad():
            f_rot, f_ph = self.net(self.t, nst, nast)
            t_rot, t_ph = self.net(self.p, st, ast)
            t_rot[rows, act[:, 0]] = rw + self.discount * f_rot.max(dim=1).values * ~dn
            t_ph[rows, act[:, 1]] = rw + self.discount * f_ph.max(dim=1).values * ~dn
        q_rot, q_ph = self.net(self.p, st, ast)
        loss = Fn.mse_loss(q_rot, t_rot) + Fn.mse_loss(q_ph, t_ph)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss


def iters_for(fn, budget_ms):
    """Warms `fn` up and sizes a timed loop to about budget_ms."""
    return max(5, min(8000, int(budget_ms / max(float(BL.per_block([fn], 5, warmup=3)[0, 0]), 1e-3))))


def replay(N, F, dev, seed=3):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(s, device=dev, generator=g)  # noqa: E731
    st, nst = (r(N, F) < 0.2).float() * r(N, F), (r(N, F) < 0.2).float() * r(N, F)
    return (st, r(N, 2), torch.randint(0, 3, (N, 2), device=dev, generator=g), r(N) * 2 - 0.5, nst, r(N, 2), r(N) < 0.1), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget-ms", type=float, default=300.0, help="timed steps per case and round")
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--loop", type=int, default=0, help="only run this many step()s at --B (for a profiler run)")
    ap.add_argument("--B", type=int, default=264)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    F = 294
    arrays, g = replay(args.rows, F, dev)
    if args.loop:
        tr = ReworkTrainer(F, dev, seed=1)
        idx = torch.randint(0, args.rows, (args.B,), device=dev, generator=g)
        for _ in range(args.loop):
            tr.step(arrays, idx, keep_grads=False)
        torch.cuda.synchronize()
        return
    out = []
    for B in (264, 4096):
        idx = torch.randint(0, args.rows, (B,), device=dev, generator=g)
        tr = ReworkTrainer(F, dev, seed=1)
        eager = Eager(tr.state_dict())
        cases = {"step": lambda: tr.step(arrays, idx, keep_grads=False), "grad": lambda: tr.grad(arrays, idx),
                 "eager_fp32": lambda: eager.step(arrays, idx)}
        iters = {k: iters_for(fn, args.budget_ms) for k, fn in cases.items()}
        # alternating: every round times every case once, a synchronise after each
        t = BL.per_block(list(cases.values()), list(iters.values()), rounds=args.rounds, sync_blocks=True)
        ms, med = dict(zip(cases, t.tolist())), dict(zip(cases, BL.median(t).tolist()))
        row = dict(B=B, F=F, launches=tr.launches(B), rounds=args.rounds, iters=iters,
                   **{k + "_ms": round(v, 4) for k, v in med.items()},
                   **{k + "_range_ms": [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in ms},
                   eager_over_step=round(med["eager_fp32"] / med["step"], 2))
        out.append(row)
        print("B %d: step %.4f ms [%.4f, %.4f] | grad %.4f ms | eager torch fp32 %.3f ms [%.3f, %.3f] (x%.1f)"
              % (B, med["step"], min(ms["step"]), max(ms["step"]), med["grad"], med["eager_fp32"], min(ms["eager_fp32"]),
                 max(ms["eager_fp32"]), row["eager_over_step"]), flush=True)
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
