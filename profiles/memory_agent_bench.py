#!/usr/bin/env python3
"""Times the memory agent's loop (antsrl_amd.agent.MemoryAgent) at c3's batch, 1024 envs x 512 ants, F = 294 (7 x 7 x 6),
power 5, mem 20, on the device:

  record     antsrl_replay_record_pre + _post at K = M (ring of M rows, for this case only) and at K = 4096 (ring of
             50 000), against the same rows recorded the way the tree offered before — a clone of the observation buffer
             before the step, then DeviceReplayMemory.extend (at K < M on rows gathered with the restated indices) —
             in the same process, alternating.  Bytes moved are computed from the shapes; the rate is given as a
             fraction of what antsrl_bench_copy reaches for the same byte count in this process.
  select     antsrl_agent_select (epsilon 0.1 and 1.0) next to the memory forward it follows.
  rollout    one whole MemoryAgent.rollout_step at K = 4096, minibatch 264, and its parts timed one by one.

  --epsilon  the skip_explored sweep instead of the above (epsilon 0, 0.1, 0.5, 0.9, 1 unless values are given): per
             epsilon and precision the full forward twice (an A/A pair: its spread is what a difference must exceed), the
             tile-list forward driven by antsrl_agent_plan's list, the plan alone, and rollout_step with the switch off
             and on (one agent, the switch flipped between alternating iterations).  The yardstick is the full forward
             and the rollout_step without the switch at the same epsilon.  Default --json:
             profiles/memory_agent_skip_c3.json.

hipEvents around `--iters` warmed iterations.  Prints one line per case and a JSON summary (--json).

    python profiles/memory_agent_bench.py [--iters 200] [--json out.json]
    python profiles/memory_agent_bench.py --epsilon [--iters 100]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/memory_agent_bench.py --probe 40   # launches per step
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd.agent import MemoryAgent  # noqa: E402
from antsrl_amd.replay import DeviceReplayMemory  # noqa: E402
from benchlib import C3_E as E, C3_N as N, F  # noqa: E402
from memory_agent_ref import sample_indices  # noqa: E402

P, MEM = (7, 7, 6), 20
M = E * N


def timed(fns, iters):
    """Median ms per call of each fn in `fns`, alternating them inside one timed loop."""
    return BL.median(BL.per_call(fns, iters, 10)).tolist()


def record_bytes(K):
    """What the two halves must move for K entries: each reads and writes K observation rows, K (2 + mem) agent floats,
    and the pre half K action pairs (2 int8 read, 2 int64 written), the post half K rewards and done flags."""
    row = 2 * F * 4 + 2 * (2 + MEM) * 4
    return K * (row + 2 + 16) + K * (row + 4 + 4 + 1 + 1)


def copy_ms(nbytes, iters):
    nbytes = (nbytes + 15) // 16 * 16
    a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return timed([lambda: _lib.check(lib.antsrl_bench_copy(C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), nbytes, st))],
                 iters)[0]


def bench_record(K, ring, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    d = dict(device="cuda", generator=g)
    obs0, obs1 = torch.rand((M, F), **d), torch.rand((M, F), **d)
    ast0, ast1 = torch.rand((M, 2), **d), torch.rand((M, 2), **d)
    m0, m1 = torch.rand((M, MEM), **d), torch.rand((M, MEM), **d)
    rot = torch.randint(-1, 2, (M,), **d).to(torch.int8)
    ph = torch.randint(0, 3, (M,), **d).to(torch.int8)
    rew, done = torch.randn((M,), **d), (torch.rand((E,), **d) < 0.1).to(torch.uint8)
    new, old = DeviceReplayMemory(ring, P, [2 + MEM], [2]), DeviceReplayMemory(ring, P, [2 + MEM], [2])
    idx = None if K == M else torch.from_numpy(sample_indices(1, 0, 0, M, K)).cuda()

    def fused():
        new.record_pre(obs0, ast0, m0, rot, ph, n_envs=E, n_ants=N, k=K, seed=1, step=0)
        new.record_post(obs1, ast1, m1, rew, done)

    def parent():
        kept, kept_ast = obs0.clone(), torch.cat([ast0, m0], 1)  # before the step: the environment overwrites obs
        nast = torch.cat([ast1, m1], 1)
        dn = done.repeat_interleave(N)
        if idx is None:
            old.extend(kept, kept_ast, (rot.long() + 1, ph.long()), rew, obs1, nast, dn)
        else:
            old.extend(kept[idx], kept_ast[idx], (rot.long()[idx] + 1, ph.long()[idx]), rew[idx], obs1[idx], nast[idx], dn[idx])

    t_new, t_old = timed([fused, parent], iters)
    for k in ("states", "actions", "rewards", "new_states", "new_agent_states", "dones", "agent_states"):
        assert torch.equal(getattr(new, k), getattr(old, k)), k  # the same rows, bit for bit
    by = record_bytes(K)
    t_copy = copy_ms(by // 2, iters)  # a copy of n bytes moves 2 n
    return dict(K=K, ring=ring, record_ms=t_new, clone_extend_ms=t_old, speedup=t_old / t_new, bytes=by,
                gbytes_per_s=by / t_new * 1e-6, copy_ms_same_bytes=t_copy, fraction_of_copy_rate=t_copy / t_new)


def bench_skip(env, ag, epsilons, iters):
    """The skip_explored sweep (module docstring)."""
    from antsrl_amd.policy import MemoryPolicy
    obs, ast = env.obs, env.agent_state
    old, new = ag._mem
    lib, st = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    T = (M + 31) // 32
    tiles, n_live = torch.zeros((T,), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    pols = dict(bf16=ag.policy, fp32=MemoryPolicy(F, "cuda", power=ag.power, mem_size=MEM, seed=1, precision="fp32"))
    for _ in range(20):  # fill the ring past min_replay: every timed step trains
        ag.rollout_step(env)
    rows = []
    for eps in epsilons:
        plan = lambda: _lib.check(lib.antsrl_agent_plan(1, 0, 0, E, N, eps, p(tiles), p(n_live), st))  # noqa: E731
        plan()
        live = int(n_live.item())
        row = dict(epsilon=eps, tiles=T, live_tiles=live, live_fraction=live / T)
        for name, pol in pols.items():
            full = lambda: pol.act(obs, ast, memory=old, out=new)  # noqa: E731
            listed = lambda: pol.act(obs, ast, memory=old, out=new, tiles=(tiles, n_live))  # noqa: E731
            t_a, t_b, t_tiles, t_plan = timed([full, full, listed, plan], iters)
            t_full = 0.5 * (t_a + t_b)
            row[name] = dict(full_forward_ms=[t_a, t_b], aa_spread_ms=abs(t_a - t_b), tile_forward_ms=t_tiles, plan_ms=t_plan,
                             fraction_times_full_plus_plan_ms=row["live_fraction"] * t_full + t_plan,
                             plan_plus_tile_forward_ms=t_plan + t_tiles)
            print("eps %.1f %s: full forward %.4f / %.4f ms (A/A) | tile-list forward %.4f ms + plan %.4f ms | live %d / %d = "
                  "%.3f -> fraction x full + plan %.4f ms" % (eps, name, t_a, t_b, t_tiles, t_plan, live, T, row["live_fraction"],
                                                              row[name]["fraction_times_full_plus_plan_ms"]), flush=True)
        ag.epsilon = eps

        def step(skip):
            ag.skip_explored = skip
            ag.rollout_step(env)

        t_off, t_off2, t_on = timed([lambda: step(False), lambda: step(False), lambda: step(True)], iters)
        row["rollout_step_ms"] = dict(off=[t_off, t_off2], on=t_on)
        print("eps %.1f rollout_step: off %.4f / %.4f ms (A/A) | on %.4f ms" % (eps, t_off, t_off2, t_on), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--epsilon", type=float, nargs="*", default=None,
                    help="the skip_explored sweep over these epsilons (none given: 0 0.1 0.5 0.9 1)")
    ap.add_argument("--skip-explored", action="store_true", help="with --probe: the agent runs with skip_explored=True")
    ap.add_argument("--probe", type=int, default=0, help="run this many rollout_steps at K = 4096 and exit (for rocprofv3)")
    a = ap.parse_args()
    env = BL.c3_env()
    ag = MemoryAgent(epsilon=0.1, discount=0.99, learning_rate=1e-5, record_per_step=4096, seed=1,
                     skip_explored=a.skip_explored)
    ag.setup(env)
    ag.initialize(env)
    env.observe()
    if a.probe:
        ag.run(env, a.probe)
        torch.cuda.synchronize()
        print("probe: %d rollout steps, %d training steps" % (a.probe, ag.trainer.step_count))
        return
    out = dict(device=torch.cuda.get_device_name(0), iters=a.iters, batch=[E, N], n_features=F)
    if a.epsilon is not None:
        out["skip_explored"] = bench_skip(env, ag, a.epsilon or [0.0, 0.1, 0.5, 0.9, 1.0], a.iters)
        return BL.write_json(out, a.json or os.path.join(ROOT, "profiles", "memory_agent_skip_c3.json"))
    out["record"] = [bench_record(M, M, max(20, a.iters // 4)), bench_record(4096, 50000, a.iters)]
    for r in out["record"]:
        print("record K = %6d: pre + post %.4f ms | clone + extend %.4f ms (%.1fx) | %.0f MB at %.0f GB/s = %.2f of the "
              "copy kernel's rate (%.4f ms)" % (r["K"], r["record_ms"], r["clone_extend_ms"], r["speedup"], r["bytes"] * 1e-6,
                                                r["gbytes_per_s"], r["fraction_of_copy_rate"], r["copy_ms_same_bytes"]), flush=True)
    # ---- select next to the forward it follows
    obs, ast = env.obs, env.agent_state
    old, new = ag._mem
    pol = ag.policy

    def forward():
        return pol.act(obs, ast, memory=old, out=new)

    rot, ph, _ = forward()
    lib, st = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sel = lambda eps: (lambda: _lib.check(lib.antsrl_agent_select(1, 0, 0, E, N, eps, 3, 3, MEM, p(rot), p(ph), p(old), p(new),  # noqa: E731
                                                                  None, st)))
    t_fwd, t_s01, t_s1 = timed([forward, sel(0.1), sel(1.0)], a.iters)
    out["select"] = dict(forward_ms=t_fwd, select_eps_0p1_ms=t_s01, select_eps_1_ms=t_s1)
    print("memory forward %.4f ms | select eps 0.1 %.4f ms, eps 1.0 %.4f ms" % (t_fwd, t_s01, t_s1), flush=True)
    # ---- the whole step and its parts
    for _ in range(20):  # fill the ring past min_replay: every timed step trains
        ag.rollout_step(env)
    rm = ag.replay_memory
    kw = ag._record_kw()
    parts = dict(
        forward=forward,
        select=sel(0.1),
        record_pre=lambda: (rm.record_pre(obs, ast, new, rot.view(-1), ph.view(-1), **kw), setattr(rm, "_pending", None)),
        env_step=lambda: env.step_update(rot, ph),
        train=lambda: ag.trainer.train(rm, False, minibatch=264, min_replay=1000, generator=ag.generator),
    )
    t_parts = dict(zip(parts, timed(list(parts.values()), a.iters)))
    t_step = timed([lambda: ag.rollout_step(env)], a.iters)[0]
    out["rollout"] = dict(K=4096, minibatch=264, rollout_step_ms=t_step, parts_ms=t_parts,
                          parts_sum_ms=sum(t_parts.values()) + t_parts["record_pre"])
    print("rollout_step %.4f ms | parts %s (record_post ~ record_pre) sum %.4f ms" % (
        t_step, {k: round(v, 4) for k, v in t_parts.items()}, out["rollout"]["parts_sum_ms"]), flush=True)
    BL.write_json(out, a.json)


if __name__ == "__main__":
    main()
