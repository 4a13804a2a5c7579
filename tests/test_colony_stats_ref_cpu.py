"""tests/stats_ref.py implements the order of sums include/antsrl.h states for the colony statistics: on inputs whose
float64 sum depends on the order (BIG = 2^60, whose ulp is 256: BIG + v == BIG for every |v| < 128) its bits are the ones
worked out by hand below, and they differ from a plain ascending sum and from a pairwise sum — so a device that sums in
another order cannot pass tests/test_gpu_colony_stats.py.  The tails (G = 156, 4096, 4097, 8240, 256 * 4096 + 1), the
exact counts and the -1 rule of the explored word per reward kind.  Of the product only its constants are read: the
reward kinds, and the word order antsrl_amd/stats.py decodes a row by, which must be the restated one."""
from types import SimpleNamespace

import numpy as np
import pytest

import stats_ref as S
from antsrl_amd import stats as product

BIG = 2.0 ** 60


def ascending(x):
    acc = 0.0
    for v in np.asarray(x, dtype=np.float64)[np.asarray(x) != 0]:  # (adding a zero changes no bit of a non-zero sum)
        acc = acc + float(v)
    return acc


def pairwise(x):
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 1:
        return float(x[0])
    h = len(x) // 2
    return pairwise(x[:h]) + pairwise(x[h:])


def grid(G, cells):
    x = np.zeros(G, dtype=np.float64)
    for g, v in cells.items():
        x[g] = v
    return x


# G -> (cells, the sum by hand)
HAND = {
    # one short segment, 156 slots in use.  Slot 27 = BIG, 28 = -BIG, 155 = 1.  s = 128: slot 27 += slot 155 -> BIG + 1 =
    # BIG; s = 16: slot 11 += 27, slot 12 += 28; s = 8: slot 3 += 11, slot 4 += 12; s = 4: slot 0 += 4 (-BIG); s = 2: slot 1
    # += 3 (BIG); s = 1: -BIG + BIG = 0.  (ascending: BIG - BIG + 1 = 1)
    156: ({27: BIG, 28: -BIG, 155: 1.0}, 0.0),
    # one whole segment.  Slot 255 takes cell 255 (BIG) and then cell 4095 (1): BIG; s = 128: slot 127 (-BIG) += slot 255 -> 0.
    4096: ({127: -BIG, 255: BIG, 4095: 1.0}, 0.0),
    # a segment and a tail of one cell.  Segment 0: slot 0 = BIG, slot 1 = -BIG, slot 2 = 3: s = 2: BIG + 3 = BIG; s = 1: 0.
    # Segment 1: 1.  Second stage: slot 0 = 0, slot 1 = 1 -> 1.  (ascending: BIG - BIG + 3 + 1 = 4)
    4097: ({0: BIG, 1: -BIG, 2: 3.0, 4096: 1.0}, 1.0),
    # two segments and a tail of 48.  Segment 0: slot 0 takes the cells 0, 256, 512, 768 = BIG, 1, -BIG, 1 -> ((BIG + 1) -
    # BIG) + 1 = 1; slot 1 = 1; slot 128 = 0.5: s = 128: slot 0 = 1.5; s = 1: 1.5 + 1 = 2.5.  Segment 1: slot 0 = -BIG,
    # slot 1 = BIG, slot 2 = 3: s = 2: -BIG + 3 = -BIG; s = 1: 0.  Segment 2 (48 cells): slot 0 = 0.25, slot 47 = 7 -> 7.25.
    # Second stage: slots 2.5, 0, 7.25: s = 2: 9.75; s = 1: 9.75.  (ascending: 1, then 1 - BIG = -BIG, + BIG = 0, + 3 + 0.25 +
    # 7 = 10.25)
    8240: ({0: BIG, 1: 1.0, 128: 0.5, 256: 1.0, 512: -BIG, 768: 1.0, 4096: -BIG, 4097: BIG, 4098: 3.0, 8192: 0.25, 8239: 7.0}, 9.75),
    # 257 segments: the second stage's slot 0 takes the partials of the segments 0 and 256: BIG + 1 = BIG; slot 1 = -BIG;
    # s = 1: 0.  (ascending: BIG - BIG + 1 = 1)
    256 * 4096 + 1: ({0: BIG, 4096: -BIG, 256 * 4096: 1.0}, 0.0),
}


@pytest.mark.parametrize("G", sorted(HAND))
def test_the_order_of_the_sums_by_hand(G):
    cells, want = HAND[G]
    x = grid(G, cells)
    got = S.cell_sum(x)
    assert S.bits(got) == S.bits(want), (G, got, want)
    assert S.segment_partials(x).shape == (-(-G // 4096),)
    assert ascending(x) != got, "the input does not tell the stated order from an ascending sum"
    if G == 8240:
        assert pairwise(x) != got and pairwise(x) != ascending(x), "nor from a pairwise one"


def test_fold_slots_is_the_monitors_rule_for_the_ants():
    """food_carried: slot t takes the ants t, t + 256, ...: 257 ants, ant 0 = BIG, ant 256 = 1 (both slot 0), ant 1 = -BIG."""
    h = np.zeros(257)
    h[0], h[256], h[1] = BIG, 1.0, -BIG
    assert S.bits(S.fold_slots(h)) == S.bits(0.0) and ascending(h) == 1.0
    assert S.bits(S.fold_slots(np.array([-0.0]))) == S.bits(0.0)  # a slot starts at +0.0
    assert S.fold_slots(np.ones((3, 2, 1000))).tolist() == [[1000.0] * 2] * 3  # batched over the leading axes


@pytest.mark.parametrize("G", [156, 4096, 4097, 8240, 256 * 4096 + 1])
def test_tails_and_exact_counts(G):
    """Random float32 grids: the stated order equals an exact (integer) sum where every partial sum is exact, and the counts
    are plain counts."""
    g = np.random.default_rng(G)
    food = g.integers(0, 8, size=(2, G)).astype(np.float32) * (g.random((2, G)) < 0.3)
    assert np.array_equal(S.cell_sum(food.astype(np.float64)), food.astype(np.int64).sum(axis=1).astype(np.float64))
    W = 1 if G > 10000 else 4 if G % 4 == 0 else 1
    reads = dict(timestep=np.array([5, 6], dtype=np.int32), anthill_food=np.array([1.5, 0.0]), food=food.reshape(2, W, G // W),
                 holding=np.array([[0.0, 1.0, 0.5], [0.0, 0.0, 0.0]], dtype=np.float32),
                 phero=np.stack([food, -food], axis=1).reshape(2, 2, W, G // W), explored=(food > 1).astype(np.uint8).reshape(2, W, G // W))
    r = S.rows(reads, SimpleNamespace(n_phero=2, reward_kind=S.REWARD_ALL))
    assert r.shape == (2, 11) and r.dtype == np.int64
    d = S.decode(r, 2)
    assert d["timestep"].tolist() == [5, 6] and d["anthill_food"].tolist() == [1.5, 0.0]
    assert d["food_cells"].tolist() == (food > 0).sum(axis=1).tolist() and d["explored_cells"].tolist() == (food > 1).sum(axis=1).tolist()
    assert d["food_carried"].tolist() == [1.5, 0.0] and d["n_carrying"].tolist() == [2, 0]
    assert np.array_equal(d["phero_mass"][:, 0], d["food_left"]) and np.array_equal(d["phero_mass"][:, 1], -d["food_left"])
    assert np.array_equal(d["phero_cells"][:, 0], d["food_cells"]) and d["phero_cells"][:, 1].tolist() == [0, 0]  # > 0, not != 0


def test_the_explored_word_is_minus_one_without_a_map():
    from antsrl_amd import config as cm
    assert (S.REWARD_EXPLORATION, S.REWARD_ALL) == (cm.REWARD_EXPLORATION, cm.REWARD_ALL)
    reads = dict(timestep=np.zeros(1, np.int32), anthill_food=np.zeros(1), food=np.zeros((1, 12, 13), np.float32),
                 holding=np.zeros((1, 4), np.float32), phero=np.zeros((1, 1, 12, 13), np.float32),
                 explored=np.ones((1, 12, 13), np.uint8))
    for kind in (cm.REWARD_NONE, cm.REWARD_EXPLORATION, cm.REWARD_FOOD, cm.REWARD_ALL):
        word = S.rows(reads, SimpleNamespace(n_phero=1, reward_kind=kind))[0, 6]
        assert word == (156 if kind in (cm.REWARD_EXPLORATION, cm.REWARD_ALL) else -1), kind


def test_the_products_word_order_is_the_restated_one():
    assert tuple(n for n, _ in product.WORDS) == S.WORDS
    d = S.decode(np.arange(22, dtype=np.int64).reshape(2, 11), 2)
    for k, (name, dtype) in enumerate(product.WORDS):
        assert d[name].dtype == np.dtype(dtype) and d[name].view(np.int64).tolist() == [k, 11 + k], name
    assert d["phero_mass"].dtype == np.float64 and d["phero_mass"].view(np.int64).tolist() == [[7, 9], [18, 20]]
    assert d["phero_cells"].tolist() == [[8, 10], [19, 21]]


def test_layout():
    assert S.layout(1, 2, 156, 1) == (88, 56, 144)
    assert S.layout(9, 3, 4097, 7) == (8 * 9 * 13, 8 * 9 * 2 * 9, 7 * 8 * 9 * 13 + 8 * 9 * 2 * 9)
