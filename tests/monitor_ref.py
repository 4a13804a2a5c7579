"""The training monitor restated in numpy and Python floats (include/antsrl.h, "The training monitor"), with
no import of the product: main.py's bookkeeping (:89-120, :149-152) and THE ORDER OF THE SUMS the device keeps.

    accumulate        episode_reward += reward                        (main.py:100; float64 += float32 casts, then adds)
    fold_total        slot t = +0.0 + x[t] + x[t + 256] + ...; x[i] += x[i + s] for i < s, s = 128, ..., 1; x[0]
    report            {total, min, max} per environment               (main.py:115-120)
    RunningLoss       main.py:106-109 in Python floats
    MonitorRef        the whole monitor: step / end_episode, the stale mean_reward of an episode without a report
    epsilon_schedule  main.py:149
"""
import math

import numpy as np

SLOTS = 256


def accumulate(episode_reward, reward):
    """episode_reward (float64) += reward, in place: numpy casts a float32 reward to float64 and adds."""
    episode_reward += np.asarray(reward).astype(np.float64)
    return episode_reward


def fold_total(x):
    """The sum of the 1-d float64 array x in the device's order."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    slots = np.zeros(SLOTS, dtype=np.float64)  # +0.0
    for k in range(0, len(x), SLOTS):          # slot t adds x[t], x[t + 256], ... ascending
        chunk = x[k: k + SLOTS]
        slots[: len(chunk)] = slots[: len(chunk)] + chunk
    s = SLOTS // 2
    while s >= 1:
        slots[:s] = slots[:s] + slots[s: 2 * s]
        s //= 2
    return slots[0]


def report(episode_reward):
    """[E][3] = {total, min, max} of episode_reward[e][:]."""
    er = np.asarray(episode_reward, dtype=np.float64)
    return np.array([[fold_total(row), row.min(), row.max()] for row in er], dtype=np.float64)


def grand_total(rep):
    """The environments' totals of one report, folded by the same rule."""
    return fold_total(np.asarray(rep)[:, 0])


class RunningLoss:
    """avg_loss of main.py:59, :106-109: None, then the first loss, then 0.99 * avg_loss + 0.01 * loss (Python floats; a
    float32 loss enters as its exact double)."""

    def __init__(self):
        self.avg, self.n, self.last = None, 0, None

    def update(self, loss):
        loss = float(loss)
        self.avg = loss if self.avg is None else 0.99 * self.avg + 0.01 * loss
        self.n += 1
        self.last = loss
        return self.avg


class MonitorRef:
    """The monitor: E environments of N ants, a report at every report_every-th step of an episode."""

    def __init__(self, E, N, report_every=50):
        self.E, self.N, self.report_every = E, N, report_every
        self.episode_reward = np.zeros((E, N), dtype=np.float64)
        self.loss = RunningLoss()
        self.reports, self.report_at, self.episodes = [], [], []
        self.episode, self.s, self._last = 0, 0, None

    def step(self, reward, loss=None):
        accumulate(self.episode_reward, np.asarray(reward).reshape(self.E, self.N))
        if loss is not None:
            self.loss.update(loss)
        self.s += 1
        if self.s % self.report_every == 0:
            self._last = report(self.episode_reward)
            self.reports.append(self._last)
            self.report_at.append((self.episode, self.s))

    def end_episode(self):
        """{grand_total, avg_loss, n_losses}: grand_total from the episode's LAST report, 0 without one (main.py:90's
        mean_reward = 0 goes stale between reports)."""
        total = 0.0 if self._last is None else grand_total(self._last)
        self.episodes.append((total, self.loss.avg, self.loss.n))
        self.episode_reward[:] = 0.0
        self.episode, self.s, self._last = self.episode + 1, 0, None

    @property
    def all_reward(self):
        return np.array([t / float(self.E * self.N) for t, _, _ in self.episodes], dtype=np.float64)

    @property
    def all_loss(self):
        return np.array([np.nan if a is None else a for _, a, _ in self.episodes], dtype=np.float64)


def epsilon_schedule(episode, min_epsilon=0.01, max_epsilon=1.0):
    return max(min_epsilon, min(max_epsilon, 1.0 - math.log10((episode + 1) / 2)))


def bits(a):
    """The bit patterns of a float64 array (so that -0.0 differs from +0.0 and a NaN equals the same NaN)."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def synthetic_rewards(steps, E, N, seed):
    """float32 [steps][E][N]: mixed signs, magnitudes 1e-3 ... 1e3 (log-uniform), one value in four an exact zero, half of
    those -0.0."""
    g = np.random.default_rng(seed)
    mag = 10.0 ** g.uniform(-3.0, 3.0, size=(steps, E, N))
    r = (mag * g.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32)
    z = g.integers(0, 8, size=mag.shape)
    r[z == 0] = 0.0
    r[z == 1] = -0.0
    return r
