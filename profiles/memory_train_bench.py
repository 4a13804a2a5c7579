#!/usr/bin/env python3
"""Times one training step of the memory agent net (CollectAgentMemory.train's arithmetic, F = 294, power 5 / mem 20
and power 4 / mem 10, B in {264, 4096, 65536}) three ways on the device:

  hip        MemoryTrainer.step: antsrl_memtrain_grad + antsrl_memtrain_apply (bf16 MFMA, fp32 Adam)
  torch32    the reference's train() as eager torch fp32: no-grad target and model forwards, the TD targets written into
             the model's q, a grad forward, two MSE losses, backward, torch.optim.Adam (its default implementation)
  torch16    the same under torch.autocast(bfloat16) with Adam(fused=True)

Prints one line per case and a JSON summary (--json).  FLOPs per step, from the shapes: 2 B S for each of the target
forward, the model forward, the backward data pass (S without layer1) and the weight gradients, S = the multiply-adds
of the 9 trained layers per row (the reference's own train() runs a fourth, no-grad model forward that the device step
does not need; it is not counted).  Bytes per step: the fp32 minibatch rows (read once) and, per net, the trained
weights in bf16 plus Adam's fp32 p, m, v, g traffic.  Peaks: 2.5 PFLOP/s bf16 MFMA dense, 8 TB/s HBM.

    python profiles/memory_train_bench.py [--iters 50] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/memory_train_bench.py --probe hip     # launches
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd.policy import MEMNET_LAYERS, memnet_param_shapes  # noqa: E402
from antsrl_amd.train import MemoryTrainer  # noqa: E402
from benchlib import F  # noqa: E402

PEAK_TFLOPS, PEAK_TBS = 2500.0, 8.0


def batch(N, mem, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = dict(device="cuda", generator=g)
    st = (torch.rand((N, F), **d) < 0.3).float() * torch.rand((N, F), **d)
    ast = torch.rand((N, 2 + mem), **d) * 2 - 1
    act = torch.stack([torch.randint(0, 3, (N,), **d), torch.randint(0, 3, (N,), **d)], dim=1)
    rw = torch.randn((N,), **d)
    nst = (torch.rand((N, F), **d) < 0.3).float() * torch.rand((N, F), **d)
    nast = torch.rand((N, 2 + mem), **d) * 2 - 1
    dn = torch.rand((N,), **d) < 0.1
    return st, ast, act, rw, nst, nast, dn


class TorchTrain:
    """The reference's train() on torch tensors (eager, what a user would write)."""

    def __init__(self, sd, discount, lr, bf16):
        self.P = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items()}
        self.T = {k: v.clone() for k, v in sd.items()}
        self.discount, self.bf16 = discount, bf16
        params = list(self.P.values())
        self.opt = torch.optim.Adam(params, lr=lr, fused=True) if bf16 else torch.optim.Adam(params, lr=lr)

    @staticmethod
    def heads(W, st, ast):
        x = torch.cat([st.reshape(st.shape[0], -1), ast], dim=1)
        L = lambda n, t: Fn.linear(t, W[n + ".weight"], W[n + ".bias"])  # noqa: E731
        h = torch.relu(L("layer3", torch.relu(L("layer2", torch.relu(L("layer1", x))))))
        g = L("layer4", h) + x
        m = L("memory_layer2", L("memory_layer1", g))  # the reference's forward computes the memory head too
        L("memory_layer3", m), L("forget_layer", m)
        return L("rotation_layer3", L("rotation_layer2", L("rotation_layer1", g))), L("pheromone_layer2", L("pheromone_layer1", g))

    def step(self, b):
        st, ast, act, rw, nst, nast, dn = b
        # two autocast regions: autocast caches its bf16 weight casts per region, and a cast made under no_grad
        # would carry no grad_fn into the grad forward
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.bf16):
            fr, fp = self.heads(self.T, nst, nast)
            tr, tp = (t.float() for t in self.heads(self.P, st, ast))
            rows = torch.arange(st.shape[0], device=st.device)
            nd = ~dn
            tr[rows, act[:, 0]] = rw + self.discount * fr.float().max(dim=1).values * nd
            tp[rows, act[:, 1]] = rw + self.discount * fp.float().max(dim=1).values * nd
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.bf16):
            qr, qp = self.heads(self.P, st, ast)
            loss = Fn.mse_loss(qr.float(), tr) + Fn.mse_loss(qp.float(), tp)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.detach()


def timed(fn, iters):
    """ms per call of fn: one event pair around `iters` warmed calls."""
    return float(BL.per_block([fn], iters, warmup=5)[0, 0])


def shape_costs(power, mem, B):
    shp = memnet_param_shapes(F, power, mem, 3, 3)
    S = sum(o * i for n, (o, i) in shp.items() if n in MEMNET_LAYERS[:9])
    s1 = shp["layer1"][0] * shp["layer1"][1]
    trained = sum(o * i + o for n, (o, i) in shp.items() if n in MEMNET_LAYERS[:9])
    flops = 2.0 * B * (S + S + (S - s1) + S)
    bytes_ = B * 2 * (F + 2 + mem + F + 2 + mem + 4) + 2 * trained * 2 + trained * 4 * 7
    return flops, bytes_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--probe", choices=("hip", "torch32", "torch16"), default=None,
                    help="run --probe-steps steps of one implementation at power 5, B = 264 (rocprofv3 launch counts: "
                         "the difference of two step counts removes the setup)")
    ap.add_argument("--probe-steps", type=int, default=20)
    a = ap.parse_args()
    if a.probe:
        tr = MemoryTrainer(F, "cuda", discount=0.99, lr=1e-5)
        b = batch(264, 20)
        run = tr.step if a.probe == "hip" else TorchTrain(tr.state_dict(), 0.99, 1e-5, a.probe == "torch16").step
        for _ in range(a.probe_steps):
            run(b)
        torch.cuda.synchronize()
        print("probe %s: %d steps" % (a.probe, a.probe_steps))
        return
    res = []
    for power, mem in ((5, 20), (4, 10)):
        for B in (264, 4096, 65536):
            tr = MemoryTrainer(F, "cuda", discount=0.99, lr=1e-5, power=power, mem_size=mem, seed=1)
            b = batch(B, mem)
            row = dict(power=power, mem_size=mem, B=B)
            row["hip_ms"] = timed(lambda: tr.step(b), a.iters)
            sd = tr.state_dict()
            for name, bf in (("torch32", False), ("torch16", True)):
                t = TorchTrain(sd, 0.99, 1e-5, bf)
                row[name + "_ms"] = timed(lambda: t.step(b), a.iters)
            flops, by = shape_costs(power, mem, B)
            row["flops"], row["bytes"] = flops, by
            row["hip_pct_peak_flops"] = 100.0 * flops / (row["hip_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12)
            row["hip_pct_peak_bytes"] = 100.0 * by / (row["hip_ms"] * 1e-3) / (PEAK_TBS * 1e12)
            res.append(row)
            print("power %d mem %2d B %6d: hip %.3f ms | torch fp32 %.3f ms (%.1fx) | torch bf16 %.3f ms (%.1fx) | "
                  "%.2f%% of bf16 peak, %.2f%% of HBM peak" % (power, mem, B, row["hip_ms"], row["torch32_ms"],
                                                               row["torch32_ms"] / row["hip_ms"], row["torch16_ms"],
                                                               row["torch16_ms"] / row["hip_ms"], row["hip_pct_peak_flops"],
                                                               row["hip_pct_peak_bytes"]), flush=True)
            del tr, b
    out = dict(device=torch.cuda.get_device_name(0), iters=a.iters, results=res)
    BL.write_json(out, a.json)


if __name__ == "__main__":
    main()
