#!/usr/bin/env python3
"""Times checkpoint, restore and fork at config 3's and config 5's batch:

  save       antsrl_checkpoint_save into a block allocated beforehand (the whole state: every array but pol_pack)
  load       antsrl_checkpoint_load from it
  fork 1     antsrl_fork_envs of environment 0 over environment 1
  fork all   antsrl_fork_envs of environment 0 over all the others (n_envs - 1 pairs: one launch per 640 pairs)

each beside antsrl_bench_copy — the library's plain 16-bytes-per-lane copy — on the same number of bytes, the two alternating
inside one timed loop.  hipEvents around `--iters` warmed calls, medians; GB/s counts read + written bytes, as bench.py's
copy figure does.  `checkpoint()` / `restore()` are also timed whole (the allocation of the block and the clones / copies of
the outputs included).  Prints one line per case and a JSON summary (--json).

    python profiles/checkpoint_bench.py [--iters 30] [--configs c3 c5] [--json profiles/checkpoint_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib as BL  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.batched import BatchedAntsEnv  # noqa: E402
from antsrl_amd.checkpoint import checkpoint_map  # noqa: E402
from bench import CONFIGS, device_identity  # noqa: E402


def timed(fns, iters):
    """Median ms per call of each fn in `fns`, alternating them inside one timed loop."""
    return BL.median(BL.per_call(fns, iters, 3)).tolist()


def run(name, iters):
    w = CONFIGS[name]
    E = w["E"]
    bf16 = w.get("policy") == "mlp"
    cfg = cm.make_cfg(E, w["N"], w["W"], w["H"], n_rocks=w["R"], deposit_strength=256.0)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16 if bf16 else torch.float32)
    lib, dev = env.lib, env.device
    env.generate(cm.make_gen(), episode_seed=1)
    env.observe()
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for _ in range(20):  # (the copies do not care what the state holds; a few steps so that it is one a user would save)
        env.step_update(torch.randint(-1, 2, (E, w["N"]), device=dev, generator=g).to(torch.int8),
                        torch.randint(0, 3, (E, w["N"]), device=dev, generator=g).to(torch.int8))
    entries, dev_bytes, host_bytes = checkpoint_map(cfg)
    payload = sum(bpe for _, _, bpe in entries) * E      # bytes of the arrays themselves
    per_env = sum(bpe for _, _, bpe in entries)
    block = torch.empty((dev_bytes,), dtype=torch.uint8, device=dev)
    blob = C.create_string_buffer(host_bytes)
    a = torch.empty(((payload + 15) // 16 * 16,), dtype=torch.uint8, device=dev).zero_()
    b = torch.empty_like(a)
    st = env._stream()
    i32p = C.POINTER(C.c_int32)

    def plain(nbytes):
        nbytes = (nbytes + 15) // 16 * 16
        return lambda: _lib.check(lib.antsrl_bench_copy(_lib.ptr(b), _lib.ptr(a), nbytes, st), "bench_copy")

    def fork(src, dst):
        s, d = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
        return lambda: _lib.check(lib.antsrl_fork_envs(env._h, s.ctypes.data_as(i32p), d.ctypes.data_as(i32p), len(s), st), "fork_envs")

    cases = [
        ("save", lambda: _lib.check(lib.antsrl_checkpoint_save(env._h, _lib.ptr(block), blob, st), "save"), payload),
        ("load", lambda: _lib.check(lib.antsrl_checkpoint_load(env._h, _lib.ptr(block), blob, st), "load"), payload),
        ("fork_1", fork([0], [1]), per_env),
        ("fork_all", fork([0] * (E - 1), list(range(1, E))), per_env * (E - 1)),
    ]
    out = dict(config=name, n_envs=E, n_ants=w["N"], grid=[w["W"], w["H"]], arrays=len(entries), device_block_bytes=dev_bytes,
               payload_bytes=payload, bytes_per_env=per_env, host_blob_bytes=host_bytes, cases={})
    with torch.cuda.device(dev):
        for label, fn, nbytes in cases:
            ms, ms_plain = timed([fn, plain(nbytes)], iters)
            gbs, gbs_plain = 2e-6 * nbytes / ms, 2e-6 * nbytes / ms_plain
            out["cases"][label] = dict(bytes=nbytes, ms=ms, gbs=gbs, bench_copy_ms=ms_plain, bench_copy_gbs=gbs_plain)
            print("%s %-9s %12d bytes  %8.4f ms %7.0f GB/s   antsrl_bench_copy %8.4f ms %7.0f GB/s   (%.2f of it)" % (
                name, label, nbytes, ms, gbs, ms_plain, gbs_plain, gbs / gbs_plain))
        holder = {}

        def whole_checkpoint():
            holder["ck"] = env.checkpoint()
        ms_ck, = timed([whole_checkpoint], max(3, iters // 3))
        ms_rs, = timed([lambda: env.restore(holder["ck"])], max(3, iters // 3))
        out["cases"]["env.checkpoint()"] = dict(ms=ms_ck)
        out["cases"]["env.restore()"] = dict(ms=ms_rs)
        print("%s env.checkpoint() %8.4f ms   env.restore() %8.4f ms   (block allocation and the outputs included)" % (name, ms_ck, ms_rs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--configs", nargs="+", default=["c3", "c5"], choices=sorted(CONFIGS))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "checkpoint_bench.py needs an MI355X"
    res = dict(device=device_identity(torch, torch.cuda.current_device()), iters=args.iters,
               runs=[run(n, args.iters) for n in args.configs])
    print(json.dumps(res["device"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
