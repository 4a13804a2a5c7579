"""pbt_plan (antsrl_amd/pbt.py) worked by hand: the rule of its docstring on small populations whose
plan can be read off the numbers.  Pure NumPy, no device.

The generator: numpy.random.default_rng(1) draws integers(2) = 0, 1, 1, 1, 0, 0, ... (asserted below), and every draw of
the plan at k = 2 and two factors is an integers(2).  A dst draws (src index, learning-rate factor, gap factor)."""
import numpy as np

from antsrl_amd.pbt import pbt_plan

DRAWS = [0, 1, 1, 1, 0, 0]
FACTORS = (0.8, 1.25)
WIDE = dict(lr_bounds=(1e-9, 1.0), gap_bounds=(1e-9, 1.0))
LR = np.array([1e-4, 2e-4, 3e-4, 4e-4, 5e-4, 6e-4, 7e-4, 8e-4])
DISCOUNT = np.array([0.9, 0.5, 0.8, 0.7, 0.95, 0.3, 0.6, 0.99])
FITNESS = np.array([5.0, 1.0, 9.0, 3.0, 7.0, 2.0, 8.0, 4.0])


def rng():
    return np.random.default_rng(1)


def test_the_generator_draws_what_the_hand_work_assumes():
    g = rng()
    assert [int(g.integers(2)) for _ in range(6)] == DRAWS


def test_p8_by_hand():
    """Order by fitness: 2 (9), 6 (8), 4, 0, 7, 3, 5 (2), 1 (1): top = [2, 6], bottom = {5, 1}.  dst = 1 draws 0, 1, 1:
    src = top[0] = 2, both factors 1.25.  dst = 5 draws 1, 0, 0: src = top[1] = 6, both factors 0.8."""
    src_of, lr, discount = pbt_plan(FITNESS, LR, DISCOUNT, quantile=0.25, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 2, 2, 3, 4, 6, 6, 7]
    want_lr, want_d = LR.copy(), DISCOUNT.copy()
    want_lr[1], want_lr[5] = 3e-4 * 1.25, 7e-4 * 0.8
    want_d[1], want_d[5] = 1.0 - (1.0 - 0.8) * 1.25, 1.0 - (1.0 - 0.6) * 0.8
    assert lr.tobytes() == want_lr.tobytes() and discount.tobytes() == want_d.tobytes()
    assert abs(lr[1] - 3.75e-4) < 1e-18 and abs(lr[5] - 5.6e-4) < 1e-18  # the numbers a reader expects
    assert abs(discount[1] - 0.75) < 1e-15 and abs(discount[5] - 0.68) < 1e-15


def test_survivors_are_bit_identical_and_the_inputs_are_not_modified():
    f, l, d = FITNESS.copy(), LR * (1.0 / 3.0), DISCOUNT * (1.0 / 3.0) + 0.5
    l0, d0 = l.copy(), d.copy()
    src_of, lr, discount = pbt_plan(f, l, d, quantile=0.25, factors=FACTORS, rng=rng(), **WIDE)
    assert f.tobytes() == FITNESS.tobytes() and l.tobytes() == l0.tobytes() and d.tobytes() == d0.tobytes()
    assert lr is not l and discount is not d and not np.shares_memory(lr, l) and not np.shares_memory(discount, d)
    keep = src_of == np.arange(8)
    assert keep.sum() == 6
    assert lr[keep].tobytes() == l0[keep].tobytes() and discount[keep].tobytes() == d0[keep].tobytes()
    assert (lr[~keep] != l0[~keep]).all() and (discount[~keep] != d0[~keep]).all()
    # lists go in as well as arrays
    again = pbt_plan(list(f), list(l), list(d), quantile=0.25, factors=FACTORS, rng=rng(), **WIDE)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (src_of, lr, discount)))


def test_ties_go_by_index():
    """P = 4, k = 1: members 0 and 1 tie at the top (0 wins), 2 and 3 at the bottom (3 is last)."""
    src_of, lr, _ = pbt_plan([2.0, 2.0, 1.0, 1.0], LR[:4], DISCOUNT[:4], quantile=0.25, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 1, 2, 0]
    assert lr[3] in (1e-4 * 0.8, 1e-4 * 1.25) and lr[:3].tobytes() == LR[:3].tobytes()  # member 0's rate, perturbed
    # the other way round: the tie at the top is between 2 and 3 (2 wins), at the bottom between 0 and 1 (1 is last)
    src_of, _, _ = pbt_plan([1.0, 1.0, 2.0, 2.0], LR[:4], DISCOUNT[:4], quantile=0.25, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 2, 2, 3]


def test_nan_ranks_last_and_a_nan_dst_takes_a_finite_src():
    nan = float("nan")
    src_of, lr, discount = pbt_plan([nan, 3.0, 2.0, 1.0], LR[:4], DISCOUNT[:4], quantile=0.25, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [1, 1, 2, 3]  # bottom is the NaN member, not member 3; top is member 1
    assert lr[0] in (2e-4 * 0.8, 2e-4 * 1.25) and lr[1:].tobytes() == LR[1:4].tobytes()
    # two NaN members rank by index behind every finite one; k = 2: top = [1, 2], bottom = {0, 3}
    src_of, _, _ = pbt_plan([nan, 3.0, 2.0, nan], LR[:4], DISCOUNT[:4], quantile=0.5, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [1, 1, 2, 2]  # dst 0 draws 0 -> top[0] = 1; dst 3 draws 1 -> top[1] = 2
    # all NaN: no finite src, every pair is dropped
    src_of, lr, discount = pbt_plan([nan] * 4, LR[:4], DISCOUNT[:4], quantile=0.5, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 1, 2, 3] and lr.tobytes() == LR[:4].tobytes() and discount.tobytes() == DISCOUNT[:4].tobytes()


def test_an_equal_pair_is_dropped_but_consumes_its_draws():
    """P = 8, k = 2, fitness 5 seven times and 1: the order is 0 .. 7, top = [0, 1], bottom = {6, 7}.  dst = 6 draws
    0, 1, 1: src 0, whose fitness equals its own: dropped.  dst = 7 then draws 1, 0, 0: src = top[1] = 1, factors 0.8.
    Had the dropped pair drawn nothing, dst = 7 would have drawn 0, 1, 1: src 0, factors 1.25."""
    f = [5.0] * 7 + [1.0]
    src_of, lr, discount = pbt_plan(f, LR, DISCOUNT, quantile=0.25, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 1, 2, 3, 4, 5, 6, 1]
    want_lr, want_d = LR.copy(), DISCOUNT.copy()
    want_lr[7], want_d[7] = 2e-4 * 0.8, 1.0 - (1.0 - 0.5) * 0.8
    assert lr.tobytes() == want_lr.tobytes() and discount.tobytes() == want_d.tobytes()


def test_lr_and_discount_are_clipped_at_both_bounds():
    """test_p8_by_hand's plan: unclipped, lr[1] = 3.75e-4, lr[5] = 5.6e-4, the gaps 0.25 and 0.32."""
    src_of, lr, discount = pbt_plan(FITNESS, LR, DISCOUNT, quantile=0.25, factors=FACTORS, rng=rng(), lr_bounds=(4e-4, 5e-4),
                                    gap_bounds=(0.3, 0.31))
    assert src_of.tolist() == [0, 2, 2, 3, 4, 6, 6, 7]
    assert lr[1] == 4e-4 and lr[5] == 5e-4  # the lower bound, the upper bound
    assert discount[1] == 1.0 - 0.3 and discount[5] == 1.0 - 0.31
    keep = src_of == np.arange(8)
    assert lr[keep].tobytes() == LR[keep].tobytes()  # a survivor outside the bounds is not clipped: it keeps its value


def test_k_zero_returns_the_inputs_and_draws_nothing():
    for f, q in (([3.0], 0.25), ([3.0], 1.0), (FITNESS[:3], 0.25), (FITNESS, 0.0), (FITNESS, 0.124)):
        g = rng()
        before = g.bit_generator.state
        P = len(f)
        src_of, lr, discount = pbt_plan(f, LR[:P], DISCOUNT[:P], quantile=q, factors=FACTORS, rng=g, **WIDE)
        assert g.bit_generator.state == before, (P, q)
        assert src_of.tolist() == list(range(P)) and src_of.dtype == np.int64
        assert lr.tobytes() == LR[:P].tobytes() and discount.tobytes() == DISCOUNT[:P].tobytes()
        assert not np.shares_memory(lr, LR) and not np.shares_memory(discount, DISCOUNT)


def test_k_is_lowered_until_two_k_fit():
    """Quantile 0.5 at P = 5: floor(2.5) = 2 and 4 <= 5, so k = 2: members 3 and 4 inherit, member 2 survives.  Quantile
    0.9 at P = 4: floor(3.6) = 3 is lowered to 2."""
    src_of, _, _ = pbt_plan([5.0, 4.0, 3.0, 2.0, 1.0], LR[:5], DISCOUNT[:5], quantile=0.5, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 1, 2, 0, 1]  # dst 3 draws 0 -> 0; dst 4 draws 1 -> 1
    src_of, _, _ = pbt_plan([4.0, 3.0, 2.0, 1.0], LR[:4], DISCOUNT[:4], quantile=0.9, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 1, 0, 1]
    src_of, _, _ = pbt_plan([4.0, 3.0, 2.0, 1.0], LR[:4], DISCOUNT[:4], quantile=1.0, factors=FACTORS, rng=rng(), **WIDE)
    assert src_of.tolist() == [0, 1, 0, 1]


def test_no_factor_and_a_quantile_outside_0_1_are_refused_before_any_draw():
    import pytest
    for bad in (dict(factors=()), dict(factors=FACTORS, quantile=-0.1), dict(factors=FACTORS, quantile=1.5)):
        g = rng()
        before = g.bit_generator.state
        with pytest.raises(AssertionError):
            pbt_plan(FITNESS, LR, DISCOUNT, rng=g, **dict(dict(quantile=0.25), **bad), **WIDE)
        assert g.bit_generator.state == before
