"""profiles/benchlib.py's two timing loops with real device events: the shapes they state, finite positive
samples, and as many calls as their arguments say.  No timing threshold: what the loops measure is the benches' business."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))

import benchlib as BL  # noqa: E402

pytestmark = pytest.mark.gpu

ITERS, ROUNDS, WARMUP = 3, 2, 2


@pytest.fixture
def counted():
    """Two trivial fns, a 1-element add and a 1 MiB fill, and their call counts."""
    one = torch.zeros((1,), device="cuda")
    mib = torch.empty((1 << 20,), dtype=torch.uint8, device="cuda")
    calls = [0, 0]

    def add():
        calls[0] += 1
        one.add_(1.0)

    def fill():
        calls[1] += 1
        mib.fill_(7)

    return [add, fill], calls


def test_per_call_shape_samples_and_call_count(counted):
    fns, calls = counted
    t = BL.per_call(fns, ITERS, WARMUP)
    assert t.shape == (2, ITERS) and t.dtype == np.float64
    assert np.isfinite(t).all() and (t > 0).all()
    assert calls == [WARMUP + ITERS] * 2


@pytest.mark.parametrize("sync_blocks", (False, True))
def test_per_block_shape_samples_and_call_count(counted, sync_blocks):
    fns, calls = counted
    t = BL.per_block(fns, ITERS, rounds=ROUNDS, warmup=WARMUP, sync_blocks=sync_blocks)
    assert t.shape == (2, ROUNDS) and t.dtype == np.float64
    assert np.isfinite(t).all() and (t > 0).all()
    assert calls == [WARMUP + ITERS * ROUNDS] * 2
