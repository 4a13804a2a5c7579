"""EpisodeMonitor — the bookkeeping of main.py's loop (:89-120, :151-152) on the device, one launch per step.

What the reference's driver keeps around its step: `episode_reward += reward` (:100), the running loss `avg_loss = 0.99 *
avg_loss + 0.01 * loss` (:106-109), `total_reward` every 50 steps (:115-120) and, per episode, all_loss / all_reward
(:151-152).  Kept with `float(loss)` and `reward.cpu()` that is a host synchronisation in every step of a loop built to have
none; here it is antsrl_monitor_step (include/antsrl.h, "The training monitor") behind `step`, on the stream the agent's
step runs on, and nothing is read back before `log()`.

The sums have a fixed order (antsrl_monitor.h), so a training curve is reproducible bit for bit.

    mon = EpisodeMonitor(env, report_every=50, max_reports=40 * episodes, max_episodes=episodes)
    for episode ...:
        for s in range(steps):
            loss = agent.rollout_step(env)
            mon.step(env.reward, loss)
        mon.end_episode()
    log = mon.log()          # the only synchronisation

The device block holds max_reports * n_envs * 24 bytes of reports: size max_reports to the run (a report is never
overwritten: one more than max_reports raises, and so does one more episode than max_episodes).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p


class EpisodeMonitor:
    def __init__(self, env_or_shape, report_every: int = 50, max_reports: int = 256, max_episodes: int = 1024,
                 device=None):
        """env_or_shape: a BatchedAntsEnv (or an RLApi over one), or (n_envs, n_ants)."""
        if isinstance(env_or_shape, (tuple, list)):
            E, N = (int(v) for v in env_or_shape)
        else:
            b = getattr(env_or_shape, "_backend", env_or_shape)
            E, N = b.cfg.n_envs, b.cfg.n_ants
            device = b.device if device is None else device
        assert report_every >= 1, "report_every must be >= 1"
        self._lib = _lib.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.n_envs, self.n_ants, self.report_every = E, N, int(report_every)
        self.max_reports, self.max_episodes = int(max_reports), int(max_episodes)
        self._dims = (E, N, self.max_reports, self.max_episodes)
        need = C.c_size_t()
        _lib.check(self._lib.antsrl_monitor_sizes(*self._dims, C.byref(need)), "monitor_sizes")
        self.state_bytes = need.value
        self._state = torch.empty((need.value // 8,), dtype=torch.float64, device=self.device)
        # the block's parts (include/antsrl.h), as views
        o = E * N
        self._episode_reward = self._state[:o].view(E, N)
        self._avg_loss, self._n_losses, self._last_loss = self._state[o], self._state[o + 1: o + 2].view(torch.int64)[0], self._state[o + 2]
        self._reports = self._state[o + 3: o + 3 + self.max_reports * E * 3].view(self.max_reports, E, 3)
        self._episodes = self._state[o + 3 + self.max_reports * E * 3:].view(self.max_episodes, 3)
        self.reset()

    def reset(self) -> None:
        """Everything to zero (antsrl_monitor_init): no episode, no report, no loss seen."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_monitor_init(_p(self._state), *self._dims, _lib.stream(self.device)), "monitor_init")
        self.episode = 0            # episodes ended so far
        self.episode_step = 0       # steps of the current episode so far
        self.n_reports = 0
        self._last_report = -1      # the current episode's last report slot
        self._report_at = []        # (episode, step) per report; step counts from 1, as main.py prints it

    # ---- device views: reading them synchronises nothing -------------------------------------------------------------
    @property
    def episode_reward(self) -> torch.Tensor:
        """float64 [n_envs, n_ants], main.py's episode_reward of every environment (a view of the block)."""
        return self._episode_reward

    @property
    def avg_loss(self) -> torch.Tensor:
        """0-d float64 view: the running loss (meaningful once n_losses > 0)."""
        return self._avg_loss

    @property
    def n_losses(self) -> torch.Tensor:
        """0-d int64 view: losses seen; 0 is main.py's `avg_loss is None`."""
        return self._n_losses

    @property
    def last_loss(self) -> torch.Tensor:
        return self._last_loss

    # ---- the loop ----------------------------------------------------------------------------------------------------
    def step(self, reward: torch.Tensor, loss=None) -> None:
        """main.py:100-120 for one step, in one launch.  reward: float32 [n_envs, n_ants] on the device (env.reward).
        loss: what the agent's train returned: a 0-d float32 device tensor (read on the device) or a Python number (the 0
        below min_replay: it counts, as in the reference), or None when the step has no loss (not training).  Reports when
        (s + 1) % report_every == 0, s counted from the episode's start."""
        assert reward.dtype == torch.float32 and reward.device == self.device and reward.is_contiguous() and \
            reward.numel() == self.n_envs * self.n_ants, "reward must be a dense float32 [n_envs, n_ants] tensor on the monitor's device"
        loss_dev, loss_host, has = None, 0.0, int(loss is not None)
        if torch.is_tensor(loss):
            assert loss.dtype == torch.float32 and loss.device == self.device and loss.numel() == 1, \
                "a device loss must be one float32 on the monitor's device"
            loss_dev = loss
        elif has:
            loss_host = float(loss)
        slot = -1
        if (self.episode_step + 1) % self.report_every == 0:
            slot = self.n_reports
            if slot >= self.max_reports:
                raise _lib.AntsrlError("EpisodeMonitor: report %d does not fit max_reports = %d" % (slot + 1, self.max_reports))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_monitor_step(_p(self._state), *self._dims, _p(reward), _p(loss_dev), loss_host, has,
                                                     slot, _lib.stream(self.device)), "monitor_step")
        self.episode_step += 1
        if slot >= 0:
            self.n_reports, self._last_report = slot + 1, slot
            self._report_at.append((self.episode, self.episode_step))

    def end_episode(self) -> None:
        """main.py:151-152 and :89 for the next episode: the episode's row, then episode_reward = 0.  The running loss
        carries over."""
        if self.episode >= self.max_episodes:
            raise _lib.AntsrlError("EpisodeMonitor: episode %d does not fit max_episodes = %d" % (self.episode + 1, self.max_episodes))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_monitor_end_episode(_p(self._state), *self._dims, self.episode, self._last_report,
                                                            _lib.stream(self.device)), "monitor_end_episode")
        self.episode += 1
        self.episode_step, self._last_report = 0, -1

    def log(self) -> dict:
        """The only call that synchronises: numpy arrays of what has been kept so far.
            reports        float64 [n_reports, n_envs, 3]   {total, min, max} of episode_reward per environment
            report_episode, report_step   int64 [n_reports]  where each was taken (step: the s + 1 main.py prints)
            all_reward     float64 [episodes]   main.py:152: the mean reward per ant at the episode's last report, over all
                                                environments (grand_total / (n_envs * n_ants), divided here); 0 without one
            all_loss       float64 [episodes]   main.py:151: avg_loss at the episode's end (nan while no loss was seen)
            grand_total, n_losses               the rows' other columns"""
        ep = self._episodes[:self.episode].cpu().numpy()
        rep = self._reports[:self.n_reports].cpu().numpy()
        at = np.array(self._report_at, dtype=np.int64).reshape(-1, 2)
        n_losses = ep[:, 2].astype(np.int64)
        return dict(reports=rep, report_episode=at[:, 0], report_step=at[:, 1], grand_total=ep[:, 0].copy(),
                    all_reward=ep[:, 0] / float(self.n_envs * self.n_ants),
                    all_loss=np.where(n_losses > 0, ep[:, 1], np.nan), n_losses=n_losses)
