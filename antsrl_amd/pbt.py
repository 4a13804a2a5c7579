"""Population-based training on top of the five populations (antsrl_amd/population.py): rank the members
by their episode reward, copy a winner's weights, target, Adam moments and ring over a loser's, and perturb the loser's
learning rate and discount.

    log = train_population(pop, env, gen, episodes, steps, pbt=PbtConfig(generation_every=2, quantile=0.25, seed=1))
    log["pbt"]["src_of"]     # [G, P]: who inherited from whom, generation by generation

What is here:

    PopulationFitness  a device block double [max_rows][P][3]: record(monitor) enqueues antsrl_pop_fitness ({total, min,
                       max} of every member's episode reward, in the monitor's fixed order of sums) into the next row
                       and reads nothing; rows() is the one call that synchronises, row(g) reads one row back.
    pbt_plan           who inherits from whom and with which learning rate and discount: pure NumPy, no device.
    PbtConfig          what driver.train_population(..., pbt=) takes.

The exploit itself is `_Population.exploit(src, dst, ring)`: antsrl_pop_exploit, every pair and every per-member array
in one launch.  The hyper-parameters are host values that travel by value in every launch, so the plan is made on the
host: one read of one fitness row per generation is the loop's only synchronisation.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import ptr as _p


@dataclass
class PbtConfig:
    """train_population's `pbt`: a generation after the last step of every generation_every-th episode; quantile,
    factors, lr_bounds and gap_bounds are pbt_plan's (the bounds of the learning rate and of 1 - discount); `seed` seeds
    the plan's numpy Generator; ring: the winner's ring slab goes with its weights."""
    generation_every: int = 1
    quantile: float = 0.25
    factors: Tuple[float, ...] = (0.8, 1.25)
    lr_bounds: Tuple[float, float] = (1e-6, 1e-2)
    gap_bounds: Tuple[float, float] = (1e-3, 0.5)
    seed: int = 0
    ring: bool = True

    def __post_init__(self):
        assert self.generation_every >= 1, "generation_every must be >= 1 (%r)" % (self.generation_every,)


class PopulationFitness:
    """The members' episode rewards on the device, a row per generation: double [max_rows][P][3], {total, min, max}
    (include/antsrl.h, "Population-based training": the total over a member's ants, min and max over its environments'
    totals, all in the monitor's order of sums, so a row is reproducible bit for bit).

    pop_or_geometry: a population that has been set up, or anything with P, n_envs and n_ants (population._Geometry);
    device: the block's, by default the population's."""

    def __init__(self, pop_or_geometry, max_rows: int, device=None):
        import torch
        g = getattr(pop_or_geometry, "g", pop_or_geometry)
        device = getattr(pop_or_geometry, "device", None) if device is None else device
        assert max_rows >= 1, "max_rows must be >= 1"
        self.P, self.n_envs, self.n_ants, self.max_rows = int(g.P), int(g.n_envs), int(g.n_ants), int(max_rows)
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self._lib = _lib.load()
        self._block = torch.zeros((self.max_rows, self.P, 3), dtype=torch.float64, device=self.device)
        self.n_rows = 0

    def record(self, monitor) -> int:
        """antsrl_pop_fitness of monitor.episode_reward into the next row, on the current stream: one launch, no host
        read.  Call it before monitor.end_episode(), which zeroes episode_reward.  Returns the row's index."""
        assert (monitor.n_envs, monitor.n_ants) == (self.n_envs, self.n_ants) and monitor.device == self.device, \
            "the monitor watches another batch than this block's"
        g = self.n_rows
        if g >= self.max_rows:
            raise _lib.AntsrlError("PopulationFitness: row %d does not fit max_rows = %d" % (g + 1, self.max_rows))
        import torch
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_pop_fitness(_p(monitor.episode_reward), self.n_envs, self.n_ants, self.P,
                                                    _p(self._block[g]), _lib.stream(self.device)), "pop_fitness")
        self.n_rows = g + 1
        return g

    def row(self, g: int) -> np.ndarray:
        """Row g, float64 [P, 3], read back (synchronises with the stream it was recorded on)."""
        assert 0 <= g < self.n_rows, (g, self.n_rows)
        return self._block[g].cpu().numpy()

    def rows(self) -> np.ndarray:
        """Every recorded row, float64 [n_rows, P, 3]: the one call that synchronises a loop that only records."""
        return self._block[:self.n_rows].cpu().numpy()


def pbt_plan(fitness, lr, discount, *, quantile: float = 0.25, factors: Sequence[float] = (0.8, 1.25), lr_bounds, gap_bounds,
             rng: np.random.Generator):
    """One generation's plan -> (src_of int64 [P], lr float64 [P], discount float64 [P]), new arrays; src_of[p] == p
    means member p survives.  fitness, lr, discount: [P]; the inputs are not modified.  No device is involved.

    The rule:

      k        floor(quantile * P), lowered until 2 k <= P.  k == 0 returns the inputs unchanged and draws nothing.
      order    the members ordered by (fitness is NaN, -fitness, index): NaN ranks last, ties go by index.
      top      the first k of the order; bottom: the last k.
      draws    for each dst in bottom, in ascending member index, three draws from rng, in this order:
                   src = top[rng.integers(k)]
                   f   = factors[rng.integers(len(factors))]     the learning rate's factor
                   f'  = factors[rng.integers(len(factors))]     the factor of the discount's gap, 1 - discount
      kept     a pair is kept only when fitness[src] > fitness[dst], or dst's fitness is NaN and src's is not.  A dropped
               pair has consumed its three draws and changes nothing.
      values   of a kept pair: src_of[dst] = src,
                   lr[dst]       = clip(lr[src] * f, lr_bounds)
                   discount[dst] = 1 - clip((1 - discount[src]) * f', gap_bounds)
      survivors keep their values exactly."""
    fitness = np.asarray(fitness, dtype=np.float64).reshape(-1)
    P = len(fitness)
    lr, discount = np.array(lr, dtype=np.float64).reshape(-1), np.array(discount, dtype=np.float64).reshape(-1)  # copies
    assert len(lr) == P and len(discount) == P, "fitness, lr and discount are [P]"
    assert 0.0 <= quantile <= 1.0, "quantile is a share of the members (%r)" % (quantile,)
    assert len(factors) >= 1, "factors holds at least one factor"
    src_of = np.arange(P, dtype=np.int64)
    k = int(np.floor(quantile * P))
    while 2 * k > P:
        k -= 1
    if k <= 0:
        return src_of, lr, discount
    nan = np.isnan(fitness)
    order = sorted(range(P), key=lambda p: (bool(nan[p]), 0.0 if nan[p] else -fitness[p], p))
    top, bottom = order[:k], order[P - k:]
    for dst in sorted(bottom):  # (2 k <= P: top and bottom are disjoint, so a src's values are never written)
        src = top[int(rng.integers(k))]
        f_lr = float(factors[int(rng.integers(len(factors)))])
        f_gap = float(factors[int(rng.integers(len(factors)))])
        if not (fitness[src] > fitness[dst] or (nan[dst] and not nan[src])):
            continue
        src_of[dst] = src
        lr[dst] = np.clip(lr[src] * f_lr, lr_bounds[0], lr_bounds[1])
        discount[dst] = 1.0 - np.clip((1.0 - discount[src]) * f_gap, gap_bounds[0], gap_bounds[1])
    return src_of, lr, discount
