"""Device-resident replay memory: agents/replay_memory.py:6-114 with the rolling
arrays kept as torch tensors ON THE GPU, so `agent.update_replay_memory(obs, agent_state, action, reward,
new_obs, new_agent_state, done)` (main.py:102) costs no PCIe round trip per step.

Same constructor, `extend`, `random_access`, `__len__`, `__getitem__` as the reference's
`ReplayMemory`.  Differences, both deliberate:
  * inputs may be torch tensors already on the device (numpy is accepted and uploaded);
  * a batch that crosses the end of the arrays wraps correctly.  The reference's recursive call
    (replay_memory.py:113-114) re-stacks an already stacked action array and mis-measures it, so it only
    works when batches never straddle `max_len`; this class implements the documented intent
    ("when head reaches the maximum length of arrays, it cycles back", replay_memory.py:7-9).
`random_access` draws its indices on the device (torch.randint, with replacement) instead of
`random.sample` on the host.
"""
from __future__ import annotations

import ctypes as C
from operator import attrgetter
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p


#: a ring's seven arrays, in the order every entry and every trainer takes them
RING_NAMES = ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")
ring_arrays = attrgetter(*RING_NAMES)  # ring -> the seven, as a tuple


class _Ring:
    """What the single agent's ring and the population's share: the seven arrays, `head`, `fill` and how they advance."""

    def _alloc(self, max_len: int, observation_space, agent_space, action_space, device, lead=()) -> None:
        """The seven arrays (replay_memory.py:18-24), zeroed, [*lead, max_len, ...]; head (:36) and fill (:39) at 0."""
        self.max_len, self.device = max_len, torch.device(device)
        z = lambda shape, dt: torch.zeros(list(lead) + [max_len] + list(shape), dtype=dt, device=self.device)  # noqa: E731
        self.states, self.new_states = z(observation_space, torch.float32), z(observation_space, torch.float32)
        self.agent_states, self.new_agent_states = z(agent_space, torch.float32), z(agent_space, torch.float32)
        self.actions = z(action_space, torch.int64)
        self.rewards = z([], torch.float32)
        self.dones = z([], torch.bool)
        self.head = self.fill = 0
        self._pending = None  # what a record_pre keeps for its record_post

    def __len__(self):
        return self.fill

    def _advance(self, n: int) -> None:
        """head and fill behind n new entries written from `head` on (replay_memory.py:109-112)."""
        if n > self.max_len:  # only the newest max_len entries survived: they start n - max_len rows on
            self.head = (self.head + n - self.max_len) % self.max_len
            n = self.max_len
        self.fill = min(self.max_len, max(self.fill, self.head + n))
        self.head = (self.head + n) % self.max_len


class DeviceReplayMemory(_Ring):
    def __init__(self, max_len: int, observation_space: Sequence[int], agent_space: Sequence[int],
                 action_space: Sequence[int], device="cuda"):
        self.observation_space, self.agent_space, self.action_space = observation_space, agent_space, action_space
        self._alloc(max_len, observation_space, agent_space, action_space, device)

    def _t(self, a, dtype):
        if a is None:
            return None
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype)

    def __getitem__(self, idx):
        idx = idx if torch.is_tensor(idx) else torch.as_tensor(idx, device=self.device)
        idx = idx.to(self.device)
        return (self.states[idx], self.agent_states[idx], self.actions[idx], self.rewards[idx],
                self.new_states[idx], self.new_agent_states[idx], self.dones[idx])

    def random_access(self, n: int, generator: Optional[torch.Generator] = None):
        idx = torch.randint(0, self.fill, (n,), device=self.device, generator=generator)
        return self[idx]

    def extend(self, states, agent_states, actions, rewards, new_states, new_agent_states, done):
        """replay_memory.py:83-114.  `actions` = (rotation[n], pheromone[n] or None); `done`: bool, a per-entry
        bool array [n], or a per-environment one [E] (n = E * ants: repeated over each environment's ants)."""
        rot = self._t(actions[0], torch.int64).reshape(-1)
        n = rot.shape[0]
        ph = self._t(actions[1], torch.int64).reshape(-1) if actions[1] is not None else torch.ones_like(rot)  # :100-103
        act = torch.stack((rot, ph), dim=-1)
        st = self._t(states, torch.float32).reshape([n] + list(self.observation_space))
        ast = self._t(agent_states, torch.float32).reshape([n] + list(self.agent_space))
        rw = self._t(rewards, torch.float32).reshape(n)
        nst = self._t(new_states, torch.float32).reshape([n] + list(self.observation_space))
        nast = self._t(new_agent_states, torch.float32).reshape([n] + list(self.agent_space))
        if torch.is_tensor(done) or isinstance(done, np.ndarray):
            dn = self._t(done, torch.bool).reshape(-1)
            if dn.numel() == 1:
                dn = dn.expand(n)
            elif dn.numel() != n:  # one flag per environment: repeated over that environment's ants
                if n % dn.numel() != 0:
                    raise ValueError("done has %d entries for %d transitions" % (dn.numel(), n))
                dn = dn.repeat_interleave(n // dn.numel())
        else:
            dn = torch.full((n,), bool(done), dtype=torch.bool, device=self.device)
        cut = max(0, n - self.max_len)  # only the newest max_len entries can survive
        row0, kept = (self.head + cut) % self.max_len, n - cut
        first = min(self.max_len - row0, kept)  # :97
        for dst, src in zip(ring_arrays(self), (st, ast, act, rw, nst, nast, dn)):
            src = src[cut:]
            dst[row0:row0 + first] = src[:first]
            if first < kept:  # wrap to the beginning (documented intent of :113-114)
                dst[: kept - first] = src[first:]
        self._advance(n)

    # ---- one step's transitions recorded around the environment step (antsrl_replay_record_pre / _post) ----------------
    def record_pre(self, obs, agent_state, memory, rotation, pheromone, n_envs: int, n_ants: int, k: Optional[int] = None,
                   seed: int = 0, step: int = 0, env_id_base: int = 0, n_rot: int = 3, obs_pitch: int = 0) -> None:
        """The first half of one step's `extend`, BEFORE the environment step overwrites its observation buffer: states,
        agent_states (= agent_state ++ memory) and actions (rotation + n_rot // 2, pheromone; pheromone None: 1) of `k`
        of the n_envs * n_ants transitions (None: all of them, in order) go to the rows `extend` would write next.  Which
        ants (a stratified sample keyed on seed, env_id_base, step) and the copy itself: include/antsrl.h.  All inputs are
        `memory` None: the memory-less form (agent_states rows are agent_state alone; antsrl_replay_record_pre_plain).
        device tensors: obs float32 or bfloat16, contiguous [.., P, P, K] — or, with obs_pitch (elements between two
        ants' rows), the padded buffer of a BatchedAntsEnv(obs_row_stride="line") —, agent_state float32 [M, 2],
        memory float32 [M, mem], rotation / pheromone int8 [M].  Nothing moves head or fill until record_post."""
        assert self._pending is None, "record_pre twice without record_post"
        M = n_envs * n_ants
        F = int(np.prod(self.observation_space))
        mem = 0 if memory is None else memory.shape[-1]
        A = int(np.prod(self.agent_space)) - mem
        spec = _lib.AntsRecordSpec(n_envs, n_ants, env_id_base, F, A, mem, n_rot, self._obs_format(obs), obs_pitch, 0,
                                   M if k is None else k, self.head, self.max_len, seed, step)
        self._check(obs, obs.dtype, M * (obs_pitch or F))
        self._check(agent_state, torch.float32, M * A)
        if memory is not None:
            self._check(memory, torch.float32, M * mem)
        self._check(rotation, torch.int8, M)
        if pheromone is not None:
            self._check(pheromone, torch.int8, M)
        self._record("replay_record_pre", spec, obs, agent_state, memory, rotation, pheromone, self.states, self.agent_states,
                     self.actions)
        self._pending = spec

    def _record(self, entry: str, spec, obs, agent_state, memory, *tensors) -> None:
        """antsrl_<entry>, or antsrl_<entry>_plain (which takes no memory) when `memory` is None."""
        entry, mem = (entry + "_plain", ()) if memory is None else (entry, (_p(memory),))
        with torch.cuda.device(self.states.device):
            _lib.check(getattr(_lib.load(), "antsrl_" + entry)(C.byref(spec), _p(obs), _p(agent_state), *mem, *map(_p, tensors),
                                                               _lib.stream(self.states.device)), entry)

    def record_post(self, obs, agent_state, memory, reward, done) -> None:
        """The second half, AFTER the step: rewards, new_states, new_agent_states (= agent_state ++ memory) and dones of the
        same transitions into the same rows; then head and fill advance exactly as `extend` advances them for k rows.
        reward float32 [M]; done: the environment's per-environment uint8 / bool [n_envs], or one host bool."""
        spec = self._pending
        assert spec is not None, "record_post without record_pre"
        M = spec.n_envs * spec.n_ants
        spec.obs_format = self._obs_format(obs)
        if not torch.is_tensor(done):
            done = torch.full((spec.n_envs,), 1 if done else 0, dtype=torch.uint8, device=self.states.device)
        elif done.dtype == torch.bool:
            done = done.view(torch.uint8)
        self._check(obs, obs.dtype, M * (spec.obs_pitch or spec.n_features))
        self._check(agent_state, torch.float32, M * spec.agent_dim)
        assert (memory is None) == (spec.mem_size == 0), "record_post: a memory exactly when record_pre had one"
        if memory is not None:
            self._check(memory, torch.float32, M * spec.mem_size)
        self._check(reward, torch.float32, M)
        self._check(done, torch.uint8, spec.n_envs)
        self._record("replay_record_post", spec, obs, agent_state, memory, reward, done, self.rewards, self.new_states,
                     self.new_agent_states, self.dones.view(torch.uint8))
        self._pending = None
        self._advance(int(spec.K))

    def _obs_format(self, obs) -> int:
        assert obs.dtype in (torch.float32, torch.bfloat16), obs.dtype
        return 1 if obs.dtype == torch.bfloat16 else 0  # ANTSRL_OBS_BF16 / ANTSRL_OBS_F32

    def _check(self, t, dtype, numel):
        assert torch.is_tensor(t) and t.device == self.states.device and t.dtype == dtype and t.is_contiguous() and \
            t.numel() == numel, (tuple(t.shape), t.dtype, t.device, numel)
