"""EpisodeStats — the colony's own numbers (food at the anthill, on the map and in the mandibles, explored cells, pheromone
on the map) as rows kept on the device, two launches per row.

The monitor reports the shaped reward and the loss; under All_Rewards with five weights (main.py:42) that curve says little
about the task.  What the reference's viewer prints (FOOD IN ANTHILL, gui/visualize.py:247) and the rest of the colony's
state could so far only be had through antsrl_read_state: whole grids copied to the host, with a synchronisation, per look.
A row is antsrl_stats_row (include/antsrl.h, "The colony statistics") on the stream the step runs on: every cell record is
read once, the sums have a fixed order (antsrl_stats.h), and nothing is read back before `rows()`.

    stats = EpisodeStats(env, max_rows=episodes * (steps // 50 + 1))
    for s in range(steps):
        agent.rollout_step(env)
        if (s + 1) % 50 == 0:
            stats.record()           # the state after Environment.update
    rows = stats.rows()              # the only synchronisation: {name: [n_rows, E]} numpy arrays

A row enqueues the environment's deferred update on its own (as every state read does), so the step behind it does not
fuse its update with the move.  A row is never overwritten: one more than max_rows raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from . import config as cm
from ._lib import ptr as _p

#: the words of an environment's record in front of the pheromones' pairs (include/antsrl.h): (name, dtype)
WORDS = (("timestep", np.int64), ("anthill_food", np.float64), ("food_left", np.float64), ("food_cells", np.int64),
         ("food_carried", np.float64), ("n_carrying", np.int64), ("explored_cells", np.int64))


class EpisodeStats:
    def __init__(self, env, max_rows: int, block: Optional[torch.Tensor] = None):
        """env: a BatchedAntsEnv (or an RLApi over one).  max_rows: rows the block holds; one more raises.
        block: a uint8 device tensor of at least `bytes` bytes, 8-byte aligned, to write into (default: a fresh one)."""
        b = getattr(env, "_backend", env)
        self.env, self.cfg, self.device = b, b.cfg, b.device
        self._lib = _lib.load()
        self.max_rows = int(max_rows)
        rb, sb, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _lib.check(self._lib.antsrl_stats_sizes(b._h, self.max_rows, C.byref(rb), C.byref(sb), C.byref(total)), "stats_sizes")
        self.row_bytes, self.scratch_bytes, self.bytes = rb.value, sb.value, total.value
        if block is None:
            block = torch.empty((self.bytes,), dtype=torch.uint8, device=self.device)
        if block.dtype != torch.uint8 or block.device != self.device or not block.is_contiguous() or block.numel() < self.bytes:
            raise _lib.AntsrlError("EpisodeStats: block must be a dense uint8 tensor of at least %d bytes on %s" % (self.bytes, self.device))
        self.block = block
        self.has_explored = self.cfg.reward_kind in (cm.REWARD_EXPLORATION, cm.REWARD_ALL)
        self.words_per_env = len(WORDS) + 2 * self.cfg.n_phero
        assert self.row_bytes == 8 * self.cfg.n_envs * self.words_per_env, "row layout"
        self.n_rows = 0

    def reset(self) -> None:
        """Forget the rows taken so far (the block is reused; nothing is launched)."""
        self.n_rows = 0

    def _args(self):
        return (self.env._h, _p(self.block), self.max_rows)

    def record(self) -> None:
        """The next row from the state as it stands (after Environment.update).  Two launches, no synchronisation; one
        row more than max_rows raises before anything is launched."""
        if self.n_rows >= self.max_rows:
            raise _lib.AntsrlError("EpisodeStats: row %d does not fit max_rows = %d" % (self.n_rows + 1, self.max_rows))
        with self.env._on_device():
            _lib.check(self._lib.antsrl_stats_row(*self._args(), self.n_rows, self.env._stream()), "stats_row")
        self.n_rows += 1

    def rows(self) -> Dict[str, np.ndarray]:
        """ONE device-to-host copy (the rows taken so far); numpy arrays [n_rows, E]: timestep, food_cells, n_carrying and
        explored_cells int64, anthill_food, food_left and food_carried float64; phero_mass float64 and phero_cells int64
        [n_rows, E, C].  explored_cells is absent where the reward kind keeps no explored map (the word is -1)."""
        E, Q, Cn, n = self.cfg.n_envs, self.words_per_env, self.cfg.n_phero, self.n_rows
        host = self.block[: n * self.row_bytes].cpu().numpy().view(np.int64).reshape(n, E, Q)
        out = {name: np.ascontiguousarray(host[:, :, k]).view(dtype) for k, (name, dtype) in enumerate(WORDS)}
        if not self.has_explored:
            assert (out["explored_cells"] == -1).all(), "explored_cells on a handle without an explored map"
            del out["explored_cells"]
        pairs = host[:, :, len(WORDS):].reshape(n, E, Cn, 2)
        out["phero_mass"] = np.ascontiguousarray(pairs[..., 0]).view(np.float64)
        out["phero_cells"] = np.ascontiguousarray(pairs[..., 1])
        return out
