"""EpisodeRenderer — RGB frames of a recorded episode, computed on the device (include/antsrl.h, "The episode renderer").

The reference's replay viewer (gui/visualize.py) needs pygame and a display.  The renderer draws what an EpisodeRecorder
holds — and only that: the live state is not read — with antsrl_render_frames: the viewer's colour layer (its chain of
mix_alpha calls) bit for bit, and a plain composition of background, anthill, walls, rocks and ants in integers (no
sprites, textures, heading marks or text).

    rec = EpisodeRecorder(env, env_indices=(0,), max_frames=steps)
    ...                                    # begin(), record() after every step
    ren = EpisodeRenderer(rec)             # zoom, view, ant_radius, phero_max_val: see __init__
    img = ren.render()                     # uint8 [n_frames, S, H * zoom, W * zoom, 3] on the device
    ren.save("out/episode_0000")           # frame_%05d.png, chunk by chunk

Image row py is y and column px is x, as pygame's surfarray shows the viewer's arrays.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib
from ._lib import ptr as _p

#: view bits (the viewer's view[i]): background (dirt, anthill, walls), ants, explored map, pheromones, food, rocks
VIEW_BACKGROUND, VIEW_ANTS, VIEW_EXPLORED, VIEW_PHERO, VIEW_FOOD, VIEW_ROCKS = 1, 2, 4, 8, 16, 32
ALL = 63
MAX_ZOOM = 8          # ANTSRL_RENDER_MAX_ZOOM
_MAX_GROUPS = 1 << 24  # a launch's workgroups (include/antsrl.h: the launch limits)


class EpisodeRenderer:
    def __init__(self, recorder, zoom: Optional[int] = None, view: int = ALL, ant_radius: Optional[int] = None,
                 phero_max_val: Optional[float] = None):
        """recorder: the EpisodeRecorder whose block is drawn.  zoom: pixels per cell side, 1..MAX_ZOOM (default: the
        largest that keeps the longer side within 900 pixels).  view: the viewer's toggles as bits (VIEW_*).
        ant_radius: an ant's disc in pixels (default max(1, zoom // 2)).  phero_max_val: what a pheromone byte is
        divided by (default: the configuration's max_val; a configuration without one must pass it, 255 being where the
        recorder's cast saturates)."""
        self.rec, self.cfg, self.device = recorder, recorder.cfg, recorder.device
        self._lib = _lib.load()
        c = self.cfg
        self.zoom = int(max(1, min(900 // max(c.w, c.h), MAX_ZOOM)) if zoom is None else zoom)
        self.view = int(view)
        self.ant_radius = int(max(1, self.zoom // 2) if ant_radius is None else ant_radius)
        if phero_max_val is None:
            if not c.has_max_val:
                raise _lib.AntsrlError("EpisodeRenderer: the configuration has no max_val: pass phero_max_val (255 is where the "
                                       "recorder's cast saturates)")
            phero_max_val = c.phero_max_val
        self.phero_max_val = float(phero_max_val)
        self.S = len(recorder.env_indices)
        # (sizes for both modes: this also runs the entry's checks on the options once)
        self._opts(False), self._opts(True)

    def _opts(self, layer_only: bool) -> _lib.AntsRenderOpts:
        o = _lib.AntsRenderOpts(self.zoom, self.view, self.ant_radius, int(layer_only), self.phero_max_val)
        for k, col in enumerate(self.rec.phero_colors[:4]):
            for j in range(3):
                o.phero_colors[k][j] = int(col[j])
        fe, sc = C.c_size_t(), C.c_size_t()
        _lib.check(self._lib.antsrl_render_sizes(self.rec.env._h, self.S, C.byref(o), C.byref(fe), C.byref(sc)), "render_sizes")
        self._frame_env_bytes, self._scratch_per_frame = fe.value, sc.value
        return o

    def max_count(self, layer_only: bool = False) -> int:
        """Frames one antsrl_render_frames call takes (the launch limits of include/antsrl.h)."""
        c = self.cfg
        ty = 32 if self.zoom <= 2 else 16 if self.zoom == 3 else 8 if self.zoom <= 5 else 4  # a workgroup's tile: 32 x ty cells
        groups = -(-c.w * c.h // 256) if layer_only else -(-c.w // 32) * -(-c.h // ty)
        n = max(1, min(65535, (_MAX_GROUPS - 1) // (groups * self.S)))
        return n - n % 16 if n >= 16 else n  # (a chunk's first byte of `out` stays 16-byte aligned)

    def _run(self, layer_only: bool, first: int, count: Optional[int], out: Optional[torch.Tensor]) -> torch.Tensor:
        rec, c, Z = self.rec, self.cfg, self.zoom
        count = rec.n_frames - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > rec.n_frames:
            raise _lib.AntsrlError("EpisodeRenderer: frames %d .. %d + %d are not among the %d recorded" % (first, first, count, rec.n_frames))
        shape = (count, self.S, c.w, c.h, 4) if layer_only else (count, self.S, c.h * Z, c.w * Z, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() or tuple(out.shape) != shape:
            raise _lib.AntsrlError("EpisodeRenderer: out must be a dense uint8 tensor of shape %s on %s" % (shape, self.device))
        o = self._opts(layer_only)
        step = self.max_count(layer_only)
        scratch = torch.empty((min(step, count) * self._scratch_per_frame,), dtype=torch.uint8, device=self.device)
        flat = out.view(count, -1)
        with rec.env._on_device():
            for k in range(0, count, step):
                n = min(step, count - k)
                _lib.check(self._lib.antsrl_render_frames(rec.env._h, _p(rec.block), self.S, rec.max_frames, int(rec.with_heatmap),
                                                          first + k, n, C.byref(o), _p(flat[k:]), _p(scratch), rec.env._stream()),
                           "render_frames")
        return out

    def colour_layer(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """The viewer's color_repr_img and its alpha byte: uint8 [count, S, W, H, 4] (R, G, B, alpha8) on the device, for
        frames first .. first + count - 1 of those recorded so far (default: all from `first`)."""
        return self._run(True, first, count, None)

    def render(self, first: int = 0, count: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The frames first .. first + count - 1 of those recorded so far as uint8 [count, S, H * zoom, W * zoom, 3] on
        the device (into `out` when given).  No synchronisation; as many launches as the launch limits ask for."""
        return self._run(False, first, count, out)

    def save(self, directory: str, env: int = 0, every: int = 1, chunk_frames: int = 64) -> list:
        """frame_%05d.png (numbered by the recorded frame) of every `every`-th recorded frame of slot `env` of the
        recorder's selection into `directory`.  Rendered and read back chunk_frames frames at a time."""
        from PIL import Image
        if not 0 <= env < self.S:
            raise _lib.AntsrlError("EpisodeRenderer.save: env %d is not a slot of the %d recorded environments" % (env, self.S))
        os.makedirs(directory, exist_ok=True)
        paths, n = [], self.rec.n_frames
        for first in range(0, n, chunk_frames):
            count = min(chunk_frames, n - first)
            wanted = [f for f in range(first, first + count) if f % every == 0]
            if not wanted:
                continue
            host = self.render(first, count)[:, env].cpu().numpy()
            for f in wanted:
                paths.append(os.path.join(directory, "frame_%05d.png" % f))
                Image.fromarray(host[f - first]).save(paths[-1])
        return paths
