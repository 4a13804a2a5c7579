#!/usr/bin/env python3
"""Times the rework agent's acting (ReworkPolicy.act: antsrl_policy_rework) at c5's batch, 512 envs x 512 ants, F = 294
(7 x 7 x 6), on float32 and bfloat16 observations, against, in the same process and alternating round by round:

  (i)   eager torch doing the reference's ten nn.Linear layers in fp32 plus both argmaxes on the same device tensors
        (bfloat16 observations are widened first): what a user has without this kernel;
  (ii)  LinearPolicy.act at the same shape (the bf16 MFMA kernel of the linear agent's net);
  (iii) the time the observation bytes take at antsrl_bench_copy's rate (read + written bytes of a device copy).

and the single launch of the collapse (antsrl_rework_collapse).  Every figure is the median over the rounds of a mean
over enough launches to fill a good fraction of a second.  Prints one line per case and a JSON summary.

    python profiles/rework_policy_bench.py [--rounds 5] [--json out.json]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import benchlib as BL  # noqa: E402

from antsrl_amd import _lib  # noqa: E402
from antsrl_amd.policy import LinearPolicy, ReworkPolicy  # noqa: E402


def eager_fp32(W, obs, ast):
    """CollectModelRework.forward and get_action's two torch.max calls as eager torch fp32."""
    x = torch.cat([obs.reshape(obs.shape[0], -1).float(), ast], dim=1)
    L = lambda n, t: Fn.linear(t, W[n + ".weight"], W[n + ".bias"])  # noqa: E731
    g = L("layer4", L("layer3", L("layer2", L("layer1", x))))
    q_rot = L("rotation_layer4", L("rotation_layer3", L("rotation_layer2", L("rotation_layer1", g))))
    q_ph = L("pheromone_layer2", L("pheromone_layer1", g))
    return torch.max(q_rot, dim=1).indices, torch.max(q_ph, dim=1).indices


def iters_for(fn, budget_ms):
    """Warms `fn` up and sizes a timed loop to about budget_ms."""
    return max(5, min(8000, int(budget_ms / max(float(BL.per_block([fn], 5, warmup=3)[0, 0]), 1e-3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--ants", type=int, default=512)
    ap.add_argument("--budget-ms", type=float, default=300.0, help="timed launches per case and round")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    E, N, F = args.envs, args.ants, 294
    M = E * N
    lib = _lib.load()
    st = _lib.stream(dev)
    obs32 = ((torch.rand((E, N, 7, 7, 6), device=dev) < 0.2).float() * torch.rand((E, N, 7, 7, 6), device=dev))
    ast = torch.rand((E, N, 2), device=dev)
    pol = ReworkPolicy(F, dev, seed=1)
    lin = LinearPolicy(F, dev, seed=1)
    W = pol.state_dict()
    ptrs = (C.c_void_p * 20)(*[t.data_ptr() for t in W.values()])

    def collapse():
        _lib.check(lib.antsrl_rework_collapse(C.byref(pol.shape), ptrs, _lib.ptr(pol.collapsed), st), "rework_collapse")

    out = []
    for name, obs in (("fp32 obs", obs32), ("bf16 obs", obs32.to(torch.bfloat16))):
        nbytes = obs.numel() * obs.element_size()
        assert nbytes % 16 == 0
        dst = torch.empty_like(obs)
        # (LinearPolicy.act takes bfloat16 rows only from the env that wrote them: timed on float32 alone)
        cases = {"act": lambda: pol.act(obs, ast), "eager_fp32": lambda: eager_fp32(W, obs.view(M, F), ast.view(M, 2)),
                 "copy": lambda: _lib.check(lib.antsrl_bench_copy(_lib.ptr(dst), _lib.ptr(obs), nbytes, st), "bench_copy"),
                 "collapse": collapse}
        if obs.dtype == torch.float32:
            cases["linear_policy"] = lambda: lin.act(obs, ast)
        iters = {k: iters_for(fn, args.budget_ms) for k, fn in cases.items()}
        # alternating: every round times every case once, a synchronise after each
        t = BL.per_block(list(cases.values()), list(iters.values()), rounds=args.rounds, sync_blocks=True)
        ms, med = dict(zip(cases, t.tolist())), dict(zip(cases, BL.median(t).tolist()))
        copy_gbs = 2 * nbytes / med["copy"] / 1e6            # read + written bytes
        obs_at_copy_ms = nbytes / copy_gbs / 1e6             # (iii)
        row = dict(obs=name, M=M, F=F, act_ms=round(med["act"], 4), act_min_ms=round(min(ms["act"]), 4),
                   act_max_ms=round(max(ms["act"]), 4), obs_read_gbs=round(nbytes / med["act"] / 1e6, 1),
                   eager_fp32_ms=round(med["eager_fp32"], 4), speedup_vs_eager=round(med["eager_fp32"] / med["act"], 2),
                   copy_gbs=round(copy_gbs, 1), obs_at_copy_rate_ms=round(obs_at_copy_ms, 4),
                   share_of_copy_rate=round(obs_at_copy_ms / med["act"], 3), collapse_ms=round(med["collapse"], 4),
                   rounds=args.rounds, iters=iters)
        if "linear_policy" in med:
            row.update(linear_policy_ms=round(med["linear_policy"], 4), act_vs_linear_policy=round(med["linear_policy"] / med["act"], 2))
        out.append(row)
        print("%s: act %.4f ms [%.4f, %.4f] (obs read at %.0f GB/s) | eager fp32 %.3f ms (x%.1f) | LinearPolicy.act %s | "
              "obs bytes at the copy rate (%.0f GB/s) %.4f ms: act runs at %.0f %% of it | collapse %.4f ms"
              % (name, med["act"], min(ms["act"]), max(ms["act"]), row["obs_read_gbs"], med["eager_fp32"],
                 row["speedup_vs_eager"], ("%.4f ms" % med["linear_policy"]) if "linear_policy" in med else "n/a (needs its env)",
                 copy_gbs, obs_at_copy_ms, 100 * row["share_of_copy_rate"], med["collapse"]), flush=True)
    BL.write_json(out, args.json)


if __name__ == "__main__":
    main()
