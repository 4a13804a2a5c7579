"""The colony statistics restated in numpy (include/antsrl.h, "The colony statistics"), with no import of the product: a
row's words from the antsrl_read_state arrays of one moment, under THE ORDER OF THE SUMS the device keeps.

    fold_slots    slot t = +0.0 + x[t] + x[t + 256] + ...; x[i] += x[i + s] for i < s, s = 128, ..., 1; x[0]
    cell_sum      the two stages: segments of 4096 canonical cells folded to partials, the partials folded by the same rule
    rows          the Q = 7 + 2 C words of every environment, as int64 bit patterns [E][Q]
    layout        row_bytes, scratch_bytes, bytes

A slot that has no cell (or no further cell) adds nothing on the device; here the input is padded with +0.0 instead.  The
two are the same bits: a slot starts at +0.0, and +0.0 + v is never -0.0, so no partial sum is a -0.0 that a +0.0 added
to it could turn into +0.0; v + (+0.0) == v for every other v (a NaN stays a NaN).
"""
import numpy as np

SLOTS, SEG = 256, 4096
REWARD_EXPLORATION, REWARD_ALL = 1, 3  # include/antsrl.h: the reward kinds that keep an explored map
WORDS = ("timestep", "anthill_food", "food_left", "food_cells", "food_carried", "n_carrying", "explored_cells")


def fold_slots(x):
    """x: float64 [..., n] -> [...]: the sum over the last axis in the device's order (256 slots, strides, the fold)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    k = max(1, -(-n // SLOTS))
    pad = np.zeros(x.shape[:-1] + (k * SLOTS,), dtype=np.float64)
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (k, SLOTS))
    slots = np.zeros(x.shape[:-1] + (SLOTS,), dtype=np.float64)  # +0.0
    for j in range(k):                                            # slot t adds x[t], x[t + 256], ... ascending
        slots = slots + pad[..., j, :]
    s = SLOTS // 2
    while s >= 1:
        slots[..., :s] = slots[..., :s] + slots[..., s: 2 * s]
        s //= 2
    return slots[..., 0]


def segment_partials(x):
    """x: float64 [..., G] (canonical cell order g = x * H + y) -> [..., nseg]."""
    x = np.asarray(x, dtype=np.float64)
    G = x.shape[-1]
    nseg = -(-G // SEG)
    pad = np.zeros(x.shape[:-1] + (nseg * SEG,), dtype=np.float64)
    pad[..., :G] = x
    return fold_slots(pad.reshape(x.shape[:-1] + (nseg, SEG)))


def cell_sum(x):
    """The sum of a grid's cells: x float64 [..., G] -> [...]."""
    return fold_slots(segment_partials(x))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def keeps_map(reward_kind):
    return int(reward_kind) in (REWARD_EXPLORATION, REWARD_ALL)


def rows(reads, cfg):
    """reads: the antsrl_read_state arrays of one moment — timestep int32 [E], anthill_food float64 [E], food float32
    [E][W][H], holding float32 [E][N], phero float32 [E][C][W][H] (materialised, as ANTSRL_S_PHERO gives it) and explored
    uint8 [E][W][H] (read only where cfg.reward_kind keeps a map).  Returns int64 [E][7 + 2 C]: every word's bits."""
    food = np.asarray(reads["food"], dtype=np.float32)
    E = food.shape[0]
    food = food.reshape(E, -1)
    phero = np.asarray(reads["phero"], dtype=np.float32)
    C = phero.shape[1]
    assert C == cfg.n_phero
    phero = phero.reshape(E, C, -1)
    holding = np.asarray(reads["holding"], dtype=np.float32).reshape(E, -1)
    out = np.zeros((E, 7 + 2 * C), dtype=np.int64)
    out[:, 0] = np.asarray(reads["timestep"]).astype(np.int64)
    out[:, 1] = bits(np.asarray(reads["anthill_food"], dtype=np.float64))
    out[:, 2] = bits(cell_sum(food.astype(np.float64)))
    out[:, 3] = (food > 0).sum(axis=1)
    out[:, 4] = bits(fold_slots(holding.astype(np.float64)))
    out[:, 5] = (holding > 0).sum(axis=1)
    if keeps_map(cfg.reward_kind):
        out[:, 6] = (np.asarray(reads["explored"]).reshape(E, -1) != 0).sum(axis=1)
    else:
        out[:, 6] = -1
    for c in range(C):
        out[:, 7 + 2 * c] = bits(cell_sum(phero[:, c].astype(np.float64)))
        out[:, 8 + 2 * c] = (phero[:, c] > 0).sum(axis=1)
    return out


def layout(E, C, G, max_rows):
    """(row_bytes, scratch_bytes, bytes)."""
    nseg = -(-G // SEG)
    row = 8 * E * (7 + 2 * C)
    scratch = 8 * E * nseg * (3 + 2 * C)
    return row, scratch, max_rows * row + scratch


def decode(words, C):
    """int64 [..., 7 + 2 C] -> {name: [...]} with the doubles viewed as float64 (phero_mass / phero_cells [..., C])."""
    words = np.ascontiguousarray(words)
    out = {}
    for k, name in enumerate(WORDS):
        col = np.ascontiguousarray(words[..., k])
        out[name] = col.view(np.float64) if name in ("anthill_food", "food_left", "food_carried") else col
    pairs = words[..., 7:].reshape(words.shape[:-1] + (C, 2))
    out["phero_mass"] = np.ascontiguousarray(pairs[..., 0]).view(np.float64)
    out["phero_cells"] = np.ascontiguousarray(pairs[..., 1])
    return out
