"""antsrl_pop_fitness restated in numpy float64 (include/antsrl.h, "Population-based training"), with no
import of the product: a member's episode reward in the monitor's order of sums (monitor_ref.fold_total).

    fitness          [P][3] = {total, min, max}: an environment's total is fold_total of its ants (slot t adds ants t,
                     t + 256, ... ascending, the 256 slots folded with s = 128 ... 1); the member's total is fold_total of
                     its Em environment totals (slot t takes environments t, t + 256, ... of the member); min and max are
                     over the environments' totals.
    ascending        the same three numbers with every sum a plain ascending one: what the order is told apart from.
    ordered_rewards  episode_reward [P Em][N] whose sums depend on their order: mixed signs, magnitudes spanning 2^40.
"""
import numpy as np

from monitor_ref import fold_total


def fitness(episode_reward, P):
    er = np.asarray(episode_reward, dtype=np.float64)
    E = er.shape[0]
    assert er.ndim == 2 and E % P == 0
    Em = E // P
    out = np.zeros((P, 3), dtype=np.float64)
    for p in range(P):
        totals = np.array([fold_total(er[e]) for e in range(p * Em, (p + 1) * Em)], dtype=np.float64)
        out[p] = fold_total(totals), totals.min(), totals.max()
    return out


def _ascending(x):
    s = np.float64(0.0)
    for v in np.asarray(x, dtype=np.float64).reshape(-1):
        s = s + v
    return s


def ascending(episode_reward, P):
    er = np.asarray(episode_reward, dtype=np.float64)
    Em = er.shape[0] // P
    out = np.zeros((P, 3), dtype=np.float64)
    for p in range(P):
        totals = np.array([_ascending(er[e]) for e in range(p * Em, (p + 1) * Em)], dtype=np.float64)
        out[p] = _ascending(totals), totals.min(), totals.max()
    return out


def ordered_rewards(P, Em, N, seed):
    """float64 [P Em][N]: sign random, magnitude 2^u with u uniform in [-20, 20): a sum of these depends on its order."""
    g = np.random.default_rng(seed)
    mag = 2.0 ** g.uniform(-20.0, 20.0, size=(P * Em, N))
    return mag * g.choice([-1.0, 1.0], size=mag.shape)
