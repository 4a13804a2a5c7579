#!/usr/bin/env python3
"""Times the episode renderer (antsrl_amd.render.EpisodeRenderer) on a recorded episode: one environment of
256 x 256 cells, 512 ants, 2 pheromones, `--frames` random-action steps recorded by an EpisodeRecorder, drawn at zoom 3
(768 x 768 pixels, 1.77 MB a frame) in chunks of `--chunk` frames into one preallocated chunk buffer.

  (a) render        EpisodeRenderer.render(first, chunk, out=...) over the whole episode: device events around the calls,
                    ms per frame; and the same for colour_layer alone
  (b) host          the same pictures the only way the parent commit could get them: EpisodeRecorder.frames() (the read-back)
                    and tests/render_ref.py in numpy, timed by the host's clock over `--host-frames` frames, which must
                    equal (a)'s bytes
  (c) bytes         the picture bytes written per second by (a), next to antsrl_bench_copy over the same byte count in
                    this process (a copy reads as many bytes as it writes; both rates are given)

Five rounds, (a) and the copy alternating inside a round; the median over the rounds and their spread, (max - min) /
median.  One process.

    python profiles/episode_renderer_bench.py [--frames 256] [--chunk 64] [--host-frames 4] [--json profiles/episode_renderer.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib as BL  # noqa: E402
import render_ref as RR  # noqa: E402
from antsrl_amd import _lib  # noqa: E402
from antsrl_amd import config as cm  # noqa: E402
from antsrl_amd.batched import BatchedAntsEnv  # noqa: E402
from antsrl_amd.recorder import EpisodeRecorder  # noqa: E402
from antsrl_amd.render import EpisodeRenderer  # noqa: E402
from antsrl_amd.synth import synth_init  # noqa: E402

W = H = 256
N, ZOOM, ROUNDS, WARMUP = 512, 3, 5, 2


def timed(fns, iters):
    """Median ms per call over ROUNDS and the spread, per function; the functions alternate inside a round, a synchronise
    after every block."""
    return BL.median_spread(BL.per_block(fns, iters, rounds=ROUNDS, warmup=WARMUP, sync_blocks=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("episode_renderer_bench: no GPU (a CPU run gives no timing)")
    cfg = cm.make_cfg(1, N, W, H, deposit_strength=256.0, max_time=max(2000, a.frames + 1))
    env = BatchedAntsEnv(cfg)
    env.reset(synth_init(cfg, seed=5, n_food_discs=20, food_rmin=5, food_rmax=10))
    rec = EpisodeRecorder(env, env_indices=(0,), max_frames=a.frames)
    g = torch.Generator(device=env.device).manual_seed(11)
    rec.begin()
    for _ in range(a.frames):
        env.step_update(torch.randint(-1, 2, (1, N), generator=g, device=env.device, dtype=torch.int8),
                        torch.randint(0, 3, (1, N), generator=g, device=env.device, dtype=torch.int8))
        rec.record()
    ren = EpisodeRenderer(rec, zoom=ZOOM)
    chunk = min(a.chunk, a.frames)
    firsts = list(range(0, a.frames - chunk + 1, chunk))
    out = torch.empty((chunk, 1, H * ZOOM, W * ZOOM, 3), dtype=torch.uint8, device=env.device)
    nbytes = out.numel()
    src = torch.empty((nbytes,), dtype=torch.uint8, device=env.device)
    lib, st = _lib.load(), env._stream()

    def render_all():
        for f in firsts:
            ren.render(f, chunk, out=out)

    def layer_all():
        for f in firsts:
            ren.colour_layer(f, chunk)

    def copy_all():
        for _ in firsts:
            _lib.check(lib.antsrl_bench_copy(C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), nbytes - nbytes % 16, st), "copy")
    (r_ms, r_sp), (c_ms, c_sp), (l_ms, l_sp) = timed([render_all, copy_all, layer_all], 3)
    n_drawn = len(firsts) * chunk
    # (b) the host's way, and the equality of the two
    k = min(a.host_frames, a.frames)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f = rec.frames()
    t1 = time.perf_counter()
    want = RR.render_frames(f, 0, k, rec.phero_colors[:cfg.n_phero], ren.phero_max_val, ZOOM, RR.VIEW_ALL, ren.ant_radius)
    t2 = time.perf_counter()
    same = bool(np.array_equal(ren.render(0, k).cpu().numpy(), want))
    res = dict(device=torch.cuda.get_device_name(0), cells=[W, H], ants=N, n_phero=cfg.n_phero, zoom=ZOOM, frames=a.frames, chunk=chunk,
               frame_bytes=nbytes // chunk,
               render_ms_per_frame=r_ms / n_drawn, render_spread=r_sp,
               colour_layer_ms_per_frame=l_ms / n_drawn, colour_layer_spread=l_sp,
               render_written_GBps=n_drawn * (nbytes // chunk) / (r_ms * 1e-3) / 1e9,
               copy_ms_per_frame=c_ms / n_drawn, copy_spread=c_sp,
               copy_written_GBps=len(firsts) * nbytes / (c_ms * 1e-3) / 1e9, copy_read_plus_written_GBps=2 * len(firsts) * nbytes / (c_ms * 1e-3) / 1e9,
               host_frames_readback_ms=(t1 - t0) * 1e3, host_render_ref_ms_per_frame=(t2 - t1) * 1e3 / k, host_frames=k,
               device_equals_host=same, kernel_source_hash=__import__("antsrl_amd.build", fromlist=["x"]).source_hash())
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    if not same:
        sys.exit("episode_renderer_bench: the device's frames differ from render_ref's")


if __name__ == "__main__":
    main()
