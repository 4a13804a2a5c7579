"""EnvCheckpoint — a batch's whole state, taken out of a BatchedAntsEnv: the device block and the host blob of
antsrl_checkpoint_save (include/antsrl.h, "CHECKPOINT") and clones of the caller-owned outputs of the last
step (obs in its dtype and pitch, agent_state, reward, done), so that an agent can act right after a restore without an
observe(), whose reward side effects would change the episode.

    ck = env.checkpoint()          # any time between two steps
    env.restore(ck)                # the same env later, or another env of the same AntsCfg (any workspace layout)
    env.fork([1, 1, 3], [0, 4, 2]) # environments copied over others inside the batch

A checkpoint does not hold the in-loop policy's pack (the agent installs it again: _DeviceAgent.load_training_state), a
caller's Reward hook state (the caller's to carry) or the bitmaps of a WALLS_INPUT generator (the env comes back without
auto-reset).  The agents' side is _DeviceAgent.training_state() / load_training_state().
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib
from .config import AntsCfg


def checkpoint_map(cfg: AntsCfg):
    """antsrl_checkpoint_map -> ([(name, offset, bytes_per_env)], device_bytes, host_bytes); host only."""
    lib = _lib.load()
    entries = (_lib.AntsCkptArray * 64)()
    n, dev, host = C.c_int32(), C.c_size_t(), C.c_size_t()
    _lib.check(lib.antsrl_checkpoint_map(C.byref(cfg), entries, 64, C.byref(n), C.byref(dev), C.byref(host)), "checkpoint_map")
    assert n.value <= 64
    return [(e.name.decode(), int(e.offset), int(e.bytes_per_env)) for e in entries[:n.value]], dev.value, host.value


class EnvCheckpoint:
    #: the tensors, in the order of save()'s file
    _TENSORS = ("block", "obs", "agent_state", "reward", "done")

    def __init__(self, cfg: AntsCfg, block: torch.Tensor, blob: bytes, obs: torch.Tensor, agent_state: torch.Tensor,
                 reward: torch.Tensor, done: torch.Tensor, auto_reset: bool = False):
        self.cfg = cfg.copy()
        self.block, self.blob = block, bytes(blob)
        self.obs, self.agent_state, self.reward, self.done = obs, agent_state, reward, done
        self.auto_reset = bool(auto_reset)  # the blob carries a generator that regenerates (BatchedAntsEnv._auto_reset)
        assert block.dtype == torch.uint8 and block.dim() == 1

    def arrays(self) -> Dict[str, torch.Tensor]:
        """The block's arrays by the carve's names: uint8 views [n_envs, bytes_per_env] (antsrl_checkpoint_map)."""
        E = self.cfg.n_envs
        return {name: self.block[off:off + E * bpe].view(E, bpe) for name, off, bpe in checkpoint_map(self.cfg)[0]}

    def save(self, path) -> None:
        """torch.save of plain tensors (on the CPU) and bytes."""
        d = {k: getattr(self, k).cpu() for k in self._TENSORS}
        d.update(blob=self.blob, cfg=bytes(self.cfg), auto_reset=self.auto_reset, format=1)
        torch.save(d, path)

    @classmethod
    def load(cls, path, device) -> "EnvCheckpoint":
        d = torch.load(path, map_location="cpu")
        if d.get("format") != 1:
            raise ValueError("%s is not an EnvCheckpoint file" % (path,))
        if len(d["cfg"]) != C.sizeof(AntsCfg):
            raise ValueError("%s holds an AntsCfg of %d bytes, this build's has %d" % (path, len(d["cfg"]), C.sizeof(AntsCfg)))
        cfg = AntsCfg.from_buffer_copy(d["cfg"])
        return cls(cfg, *(d[k].to(device) if k != "blob" else d[k]
                          for k in ("block", "blob", "obs", "agent_state", "reward", "done")), auto_reset=d["auto_reset"])
