"""The numpy restatement of the memory agent's draw specification (tests/memory_agent_ref.py) checked on its own: the
properties the header states, and the fixture fact that fixes MemoryAgent's default state_memory.  CPU only."""
import os

import numpy as np
import pytest

import memory_agent_ref as R

CONTRACT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract")


def test_k_equal_m_is_the_identity():
    for M in (1, 7, 160, 4096):
        assert np.array_equal(R.sample_indices(3, 5, 0, M, M), np.arange(M))


@pytest.mark.parametrize("M,K", [(524288, 4096), (1000, 7), (257, 256), (10, 3), (5, 1), (4096, 4095)])
def test_every_index_lies_in_its_stratum(M, K):
    for step in range(3):
        a = R.sample_indices(11, step, 2, M, K)
        j = np.arange(K)
        assert np.all(a >= j * M // K) and np.all(a < (j + 1) * M // K)
        assert np.all(np.diff(a) > 0) and a[-1] < M


def test_explore_rate_and_action_ranges():
    ex = np.stack([R.explores(9, s, 0, 64, 0.3) for s in range(64)])  # 4096 (env, step) pairs
    assert abs(ex.mean() - 0.3) <= 0.036  # 5 sigma of a Bernoulli(0.3) mean over 4096 draws
    assert not R.explores(9, 0, 0, 4096, 0.0).any() and R.explores(9, 0, 0, 4096, 1.0).all()
    rot, ph = R.random_actions(9, 0, 0, 64, 512, 3, 3)
    assert set(np.unique(rot)) == {-1, 0, 1} and set(np.unique(ph)) == {0, 1, 2}
    for v in (-1, 0, 1):
        assert abs((rot == v).mean() - 1 / 3) < 0.01 and abs((ph == v + 1).mean() - 1 / 3) < 0.01
    u = R.u01(R.draw(1, R.DRAW_SAMPLE, 0, 0, np.arange(100000)))
    assert u.min() >= 0.0 and u.max() < 1.0
    # the stream tags separate the streams: equal keys, different tags, unrelated draws
    a, b = R.draw(1, R.DRAW_ROTATION, 0, 0, np.arange(64)), R.draw(1, R.DRAW_PHEROMONE, 0, 0, np.arange(64))
    assert not np.any(a == b)


def test_shards_draw_what_the_full_batch_draws():
    E, N = 8, 16
    full_ex = R.explores(5, 3, 0, E, 0.5)
    full_r, full_p = R.random_actions(5, 3, 0, E, N, 3, 3)
    for base in (0, E // 2):
        assert np.array_equal(R.explores(5, 3, base, E // 2, 0.5), full_ex[base:base + E // 2])
        r, p = R.random_actions(5, 3, base, E // 2, N, 3, 3)
        assert np.array_equal(r, full_r[base:base + E // 2]) and np.array_equal(p, full_p[base:base + E // 2])
    rng = np.random.default_rng(0)
    rot, ph = rng.integers(-1, 2, (E, N)), rng.integers(0, 3, (E, N))
    mo, mn = rng.random((E, N, 4), np.float32), rng.random((E, N, 4), np.float32)
    whole = R.select(5, 3, 0, 0.5, 3, 3, rot, ph, mo, mn)
    h = E // 2
    for base in (0, h):
        part = R.select(5, 3, base, 0.5, 3, 3, rot[base:base + h], ph[base:base + h], mo[base:base + h], mn[base:base + h])
        for w, q in zip(whole, part):
            assert np.array_equal(w[base:base + h], q)


def test_ring_rows():
    js, rows, head = R.ring_rows(45, 50, 12)
    assert list(js) == list(range(12)) and list(rows) == [45, 46, 47, 48, 49, 0, 1, 2, 3, 4, 5, 6] and head == 7
    js, rows, head = R.ring_rows(7, 50, 64)  # K > max_len: the last 50 entries
    assert list(js) == list(range(14, 64)) and len(set(rows)) == 50 and head == 21 and rows[-1] == 20


def test_the_reference_stores_the_post_action_memory_in_both_arrays():
    z = np.load(os.path.join(CONTRACT, "memory_train_ref.npz"))
    a, b = z["rows/agent_states"], z["rows/new_agent_states"]
    assert a.shape[0] == 621 and a.shape == b.shape
    assert np.array_equal(a[:, 2:], b[:, 2:])


def test_the_agent_contract_fixture_is_what_recording_must_reproduce():
    z = np.load(os.path.join(CONTRACT, "agent_contract.npz"))
    before = np.concatenate([z["obs0"][None], z["obs"][:-1]]).astype(np.float32)
    assert np.array_equal(z["replay_states"], before.reshape((-1,) + before.shape[2:]))
    assert np.array_equal(z["replay_actions"][:, 0], z["rot"].reshape(-1) + 1)
    assert np.array_equal(z["replay_actions"][:, 1], z["ph"].reshape(-1))
    assert np.array_equal(z["replay_rewards"], z["reward"].reshape(-1).astype(np.float32))
