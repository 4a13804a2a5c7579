"""EpisodeRecorder — the snapshots of a visualised episode (main.py:67, :137-147) kept on the device, one launch per step.

main.py keeps `Environment.save_state()` after every step of the episodes it visualises and pickles the list at the
episode's end for the replay viewer.  snapshot.snapshot_batched does that through antsrl_read_state: the state arrays of
ALL environments, copied to the host, with a synchronisation, after every step.  The recorder packs what the viewer needs
of the chosen environments (uint8 grids and the ants: include/antsrl.h, "The episode recorder") into a device-resident
frame log with antsrl_recorder_frame, on the stream the step runs on, and nothing is read back before `frames()` /
`snapshots()` at the episode's end — the moment main.py pickles.

    rec = EpisodeRecorder(env, env_indices=(0,), max_frames=steps)
    rec.begin()                      # after env.generate / env.reset: the walls, the anthill, the rocks' radius and weight
    for s in range(steps):
        agent.rollout_step(env)
        rec.record()                 # the state after Environment.update, where main.py:138 takes it
    states = rec.snapshots()         # the only synchronisation: what snapshot_batched(env, env_indices) after each of
                                     # those steps would have appended, in that order

A recorded step enqueues the environment's deferred update on its own (as every state read does), so it does not fuse
with the next step's move.  The block holds max_frames frames (`frame_bytes` each: 0.28 MB per environment at 256 x 256
cells, 512 ants, 2 pheromones) and is reused by every begin().
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import config as cm
from . import snapshot
from ._lib import ptr as _p

def _a16(n: int) -> int:
    return (n + 15) // 16 * 16


class EpisodeRecorder:
    def __init__(self, env, env_indices: Sequence[int] = (0,), max_frames: Optional[int] = None, with_heatmap: bool = True,
                 phero_colors=snapshot.PHERO_COLORS, block: Optional[torch.Tensor] = None):
        """env: a BatchedAntsEnv (or an RLApi over one).  env_indices: 1..8 distinct environments, in the order their
        snapshots are wanted.  max_frames: frames the block holds (default: cfg.max_time, an episode); one more raises.
        with_heatmap: keep the reward's explored map (RLVisualization.heatmap) where the reward kind has one.
        block: a uint8 device tensor of at least `bytes` bytes, 16-byte aligned, to record into (default: a fresh one)."""
        b = getattr(env, "_backend", env)
        self.env, self.cfg, self.device = b, b.cfg, b.device
        self._lib = _lib.load()
        self.env_indices = tuple(int(e) for e in env_indices)
        self.max_frames = int(self.cfg.max_time if max_frames is None else max_frames)
        self.with_heatmap, self.phero_colors = bool(with_heatmap), phero_colors
        S = len(self.env_indices)
        self._idx = (C.c_int32 * max(S, 1))(*self.env_indices)
        st, fr, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _lib.check(self._lib.antsrl_recorder_sizes(b._h, S, self.max_frames, int(self.with_heatmap), C.byref(st), C.byref(fr),
                                                   C.byref(total)), "recorder_sizes")
        self.static_bytes, self.frame_bytes, self.bytes = st.value, fr.value, total.value
        if block is None:
            block = torch.empty((self.bytes,), dtype=torch.uint8, device=self.device)
        if block.dtype != torch.uint8 or block.device != self.device or not block.is_contiguous() or block.numel() < self.bytes:
            raise _lib.AntsrlError("EpisodeRecorder: block must be a dense uint8 tensor of at least %d bytes on %s" % (self.bytes, self.device))
        self.block = block
        c = self.cfg
        self.has_heatmap = self.with_heatmap and c.reward_kind in (cm.REWARD_EXPLORATION, cm.REWARD_ALL)
        # the layout (include/antsrl.h): (name, dtype, shape, bytes) per section, in order
        N, R, Cn, W, H = c.n_ants, c.n_rocks, c.n_phero, c.w, c.h
        Gp = _a16(W * H)
        self._static_fields = [("anthill_xyr", np.int32, (3,), 16), ("rock_rw", np.float64, (R, 2), 16 * R),
                               ("walls", np.uint8, (W, H), Gp)]
        self._frame_fields = [("timestep", np.int32, (), 16), ("anthill_food", np.float64, (), 16),
                              ("rock_centers", np.float64, (R, 2), 16 * R), ("ants_xyt", np.float64, (N, 3), _a16(24 * N)),
                              ("holding", np.float32, (N,), _a16(4 * N)), ("mandibles", np.uint8, (N,), _a16(N)),
                              ("reward_state", np.uint8, (N,), _a16(N))]
        self._frame_fields += [("phero%d" % k, np.uint8, (W, H), Gp) for k in range(Cn)] + [("food", np.uint8, (W, H), Gp)]
        if self.has_heatmap:
            self._frame_fields.append(("explored", np.uint8, (W, H), Gp))
        assert sum(f[3] for f in self._static_fields) * S == self.static_bytes, "static layout"
        assert sum(f[3] for f in self._frame_fields) * S == self.frame_bytes, "frame layout"
        self.n_frames = 0
        self._begun = False

    @property
    def static_fields(self):
        """The sections of one environment's piece of the static part, in order: (name, dtype, shape, bytes)."""
        return list(self._static_fields)

    @property
    def frame_fields(self):
        """The sections of one environment's piece of a frame, in order (pheromone plane k is "phero%d" % k)."""
        return list(self._frame_fields)

    def _args(self):
        return (self.env._h, _p(self.block), self._idx, len(self.env_indices), self.max_frames, int(self.with_heatmap))

    def begin(self) -> None:
        """A new episode: the frame counter to zero and the static part (walls, anthill, the rocks' radius and weight)
        from the state as it stands — call it after env.generate / env.reset.  One launch, no synchronisation."""
        with self.env._on_device():
            _lib.check(self._lib.antsrl_recorder_begin(*self._args(), self.env._stream()), "recorder_begin")
        self.n_frames = 0
        self._begun = True

    def record(self) -> None:
        """The next frame from the state as it stands (after Environment.update).  One launch, no synchronisation; one
        frame more than max_frames raises before anything is launched."""
        if not self._begun:
            raise _lib.AntsrlError("EpisodeRecorder.record: begin() has not been called")
        if self.n_frames >= self.max_frames:
            raise _lib.AntsrlError("EpisodeRecorder: frame %d does not fit max_frames = %d" % (self.n_frames + 1, self.max_frames))
        with self.env._on_device():
            _lib.check(self._lib.antsrl_recorder_frame(*self._args(), self.n_frames, self.env._stream()), "recorder_frame")
        self.n_frames += 1

    @staticmethod
    def _fields(buf: np.ndarray, fields) -> Dict[str, np.ndarray]:
        """buf: uint8 [..., piece bytes] -> {name: [..., *shape]} (copies)."""
        out, off = {}, 0
        for name, dtype, shape, nbytes in fields:
            used = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
            raw = np.ascontiguousarray(buf[..., off: off + used])
            out[name] = raw.view(dtype).reshape(buf.shape[:-1] + tuple(shape))
            off += nbytes
        return out

    def frames(self) -> Dict[str, np.ndarray]:
        """ONE device-to-host copy (the static part and the frames recorded so far); numpy arrays per field:
            per frame  [n_frames, S, ...]: timestep int32, anthill_food float64, rock_centers float64 [R, 2], ants_xyt
                       float64 [N, 3], holding float32 [N], mandibles / reward_state uint8 [N], phero uint8 [C, W, H],
                       food uint8 [W, H] and, with a heatmap, explored uint8 [W, H]
            static     [S, ...]: anthill_xyr int32 [3], rock_rw float64 [R, 2], walls uint8 [W, H]"""
        S, n = len(self.env_indices), self.n_frames
        host = self.block[: self.static_bytes + n * self.frame_bytes].cpu().numpy()
        out = self._fields(host[: self.static_bytes].reshape(S, -1), self._static_fields)
        fr = self._fields(host[self.static_bytes:].reshape(n, S, self.frame_bytes // S), self._frame_fields)
        Cn = self.cfg.n_phero
        fr["phero"] = np.stack([fr.pop("phero%d" % k) for k in range(Cn)], axis=2)
        out.update(fr)
        return out

    def snapshots(self) -> List[snapshot.Environment]:
        """The recorded frames as snapshots in the reference's layout (snapshot.snapshot_from_arrays): frame by frame,
        the chosen environments in their order — the list snapshot_batched(env, env_indices) called after each of the
        recorded steps would have built."""
        c, f = self.cfg, self.frames()
        rocks = c.n_rocks > 0
        out = []
        for k in range(self.n_frames):
            for s in range(len(self.env_indices)):
                out.append(snapshot.snapshot_from_arrays(
                    c.w, c.h, c.max_time, int(f["timestep"][k, s]), ants_xyt=f["ants_xyt"][k, s], mandibles=f["mandibles"][k, s],
                    holding=f["holding"][k, s], reward_state=f["reward_state"][k, s], phero=f["phero"][k, s],
                    phero_colors=self.phero_colors, phero_max_val=(c.phero_max_val if c.has_max_val else None),
                    food=f["food"][k, s], walls=f["walls"][s], anthill_xyr=f["anthill_xyr"][s],
                    anthill_food=f["anthill_food"][k, s],
                    rock_centers=f["rock_centers"][k, s] if rocks else None,
                    rock_radiuses=f["rock_rw"][s][:, 0] if rocks else None,
                    rock_weights=f["rock_rw"][s][:, 1] if rocks else None,
                    heatmap=f["explored"][k, s].astype(bool) if self.has_heatmap else None))
        return out
