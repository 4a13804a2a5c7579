#!/usr/bin/env python3
"""Times the memory agent net (antsrl_policy_memory_ex) at c3's batch: M = 524 288 ants, F = 294 (7 x 7 x 6), for
power 5 / mem_size 20 and power 4 / mem_size 10, on float32 and bfloat16 observations, against the same net written as
eager torch F.linear calls (what a user would write): bf16 for the bf16 kernel, fp32 for the fp32 one.  Prints one
line per case and a JSON summary.

    python profiles/memory_policy_bench.py [--precision bf16|fp32|both] [--iters 20] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/memory_policy_bench.py --iters 20

FLOP count: 2 x (multiply-adds of the twelve layers at their real widths) per ant.  The MFMA peaks of the MI355X are
2.5 PFLOP/s for bf16 operands and 157.3 TFLOP/s for fp32 operands (dense)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import benchlib as BL  # noqa: E402

from antsrl_amd.policy import MEMNET_LAYERS, MemoryPolicy, memnet_param_shapes  # noqa: E402

PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}


def eager_bf16(W, obs, ast, mem):
    """The net as eager torch bf16 (fp32 blend), no fusion: the code a user would write."""
    x = torch.cat([obs.reshape(obs.shape[0], -1).to(torch.bfloat16), ast.to(torch.bfloat16), mem.to(torch.bfloat16)], dim=1)
    L = lambda n, t: Fn.linear(t, W[n + ".weight"], W[n + ".bias"])  # noqa: E731
    h = torch.relu(L("layer3", torch.relu(L("layer2", torch.relu(L("layer1", x))))))
    g = L("layer4", h) + x
    q_rot = L("rotation_layer3", L("rotation_layer2", L("rotation_layer1", g)))
    q_ph = L("pheromone_layer2", L("pheromone_layer1", g))
    m = L("memory_layer2", L("memory_layer1", g))
    s = torch.sigmoid(L("forget_layer", m).float())
    new = torch.tanh(L("memory_layer3", m).float()) * s + mem * (1 - s)
    return q_rot.argmax(dim=1), q_ph.argmax(dim=1), new


def eager_fp32(W, obs, ast, mem):
    """The net as eager torch fp32, no fusion: the reference's own precision."""
    x = torch.cat([obs.reshape(obs.shape[0], -1).float(), ast, mem], dim=1)
    L = lambda n, t: Fn.linear(t, W[n + ".weight"], W[n + ".bias"])  # noqa: E731
    h = torch.relu(L("layer3", torch.relu(L("layer2", torch.relu(L("layer1", x))))))
    g = L("layer4", h) + x
    q_rot = L("rotation_layer3", L("rotation_layer2", L("rotation_layer1", g)))
    q_ph = L("pheromone_layer2", L("pheromone_layer1", g))
    m = L("memory_layer2", L("memory_layer1", g))
    s = torch.sigmoid(L("forget_layer", m))
    new = torch.tanh(L("memory_layer3", m)) * s + mem * (1 - s)
    return q_rot.argmax(dim=1), q_ph.argmax(dim=1), new


def time_ms(fn, iters):
    """ms per call of fn: one event pair around `iters` warmed calls."""
    return float(BL.per_block([fn], iters, warmup=3)[0, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ants", type=int, default=1024 * 512)
    ap.add_argument("--precision", choices=("bf16", "fp32", "both"), default="bf16")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    M, F = args.ants, 294
    g = torch.Generator(device="cpu").manual_seed(0)
    obs32 = (torch.rand((M, 7, 7, 6), generator=g) < 0.2).float().to(dev) * torch.rand((M, 7, 7, 6), device=dev)
    obs16 = obs32.to(torch.bfloat16)
    ast = torch.rand((M, 2), device=dev)
    out = []
    for prec in (("bf16", "fp32") if args.precision == "both" else (args.precision,)):
        eager, eager_name = (eager_bf16, "eager_bf16") if prec == "bf16" else (eager_fp32, "eager_fp32")
        peak = PEAK_TFLOPS[prec]
        for power, mem_size in ((5, 20), (4, 10)):
            pol = MemoryPolicy(F, dev, power=power, mem_size=mem_size, seed=1, precision=prec)
            mac = sum(o * i for o, i in memnet_param_shapes(F, power, mem_size, 3, 3).values())
            flop = 2.0 * mac * M
            W = {k: v.to(torch.bfloat16 if prec == "bf16" else torch.float32) for k, v in pol.params.items()}
            mem = torch.zeros((M, mem_size), device=dev)
            for name, obs in (("fp32 obs", obs32), ("bf16 obs", obs16)):
                mo = torch.empty_like(mem)
                ms = time_ms(lambda: pol.act(obs, ast, memory=mem, out=mo), args.iters)
                me = time_ms(lambda: eager(W, obs, ast, mem), max(3, args.iters // 4))
                tf = flop / ms / 1e9
                obs_gbs = obs.numel() * obs.element_size() / ms / 1e6
                row = dict(power=power, mem_size=mem_size, obs=name, M=M, kernel_ms=round(ms, 4), tflops=round(tf, 1),
                           peak_frac=round(tf / peak, 4), obs_read_gbs=round(obs_gbs, 1))
                row[eager_name + "_ms"] = round(me, 4)
                row.update(speedup_vs_eager=round(me / ms, 2), mac_per_ant=mac, packed_bytes=pol.packed.numel())
                if prec != "bf16":
                    row = dict(precision=prec, **row)
                out.append(row)
                print("%s power %d mem %2d %s: kernel %.3f ms (%.1f TFLOP/s, %.1f %% of the %s peak, obs %.0f GB/s) | eager "
                      "torch %s %.3f ms (x%.2f)" % (prec, power, mem_size, name, ms, tf, 100 * tf / peak, prec, obs_gbs, prec,
                                                     me, me / ms), flush=True)
            del pol
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
