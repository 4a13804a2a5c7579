"""profiles/benchlib.py without a GPU: its two timing loops do, call for call, what the benches' private loops
did; its statistics are the ones the benches computed inline; every bench imports; and no bench creates a timing event or
imports another bench.

The traces: torch.cuda.Event and torch.cuda.synchronize are replaced by fakes that log ("record", id), ("sync",) and
("call", k).  An event's id is the ordinal of its first record, so only the order of the record / call / sync entries is
compared, not where the events are constructed (memory_policy_bench.time_ms created its pair before its synchronise, the
others after).  elapsed_time is 100 x the start's position in the log plus the end's, so every pair has a value of its own: a
transposed axis or a wrong divisor shows.  PARENT holds, per private loop of the tree before benchlib, the log and the return
it gave under these fakes at the smallest arguments that reach every loop level (two fns, iters 2, warmup 1, two rounds;
time_ms's warm-up was a fixed 3); they were recorded from those functions before they were deleted."""
import ast
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles")
for _p in (PROFILES, os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import benchlib as BL  # noqa: E402

BENCHES = sorted(glob.glob(os.path.join(PROFILES, "*_bench.py"))) + [os.path.join(PROFILES, "dqn_launch_repeat.py")]
#: the one script that keeps a timing loop of its own (its docstring says why)
PRIVATE_LOOP = "episode_recorder_bench.py"
#: the one import between benches: a model, not harness
ALLOWED_IMPORT = ("joint_agent_bench", "linear_agent_bench")


class FakeCuda:
    """Installs the fakes and keeps the log."""

    def __init__(self, monkeypatch):
        self.log = log = []

        class Event:
            def __init__(self, enable_timing=False):
                assert enable_timing
                self.id = self.pos = None

            def record(self):
                if self.id is None:
                    self.id = sum(1 for e in log if e[0] == "record" and e[2])
                log.append(("record", self.id, self.pos is None))
                self.pos = len(log)

            def elapsed_time(self, end):
                return float(100 * self.pos + end.pos)

        monkeypatch.setattr(torch.cuda, "Event", Event)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: log.append(("sync",)))

    def fns(self, n):
        return [lambda k=k: self.log.append(("call", k)) for k in range(n)]

    def compact(self):
        """The log as one string: r<id> a record, c<k> a call, s a synchronise."""
        return " ".join("s" if e[0] == "sync" else e[0][0] + str(e[1]) for e in self.log)

    def calls(self, k):
        return sum(1 for e in self.log if e == ("call", k))


PARENT = {
    "linear_agent_bench.timed": dict(
        log="c0 c1 s r0 c0 r1 r2 c1 r3 r4 c0 r5 r6 c1 r7 s",
        ret=[709.0, 1012.0]),
    "population_bench.timed": dict(
        log="c0 s r0 c0 r1 r2 c0 r3 s",
        ret=456.5),
    "rework_agent_bench.rounds": dict(
        log="c0 c1 s r0 c0 c0 r1 r2 c1 c1 r3 r4 c0 c0 r5 r6 c1 c1 r7 s",
        ret=[(405.5, 0.9963008631319359), (607.5, 0.6650205761316872)]),
    "colony_stats_bench.blocks": dict(
        log="c0 c1 s r0 c0 r1 r2 c1 r3 r4 c0 r5 r6 c1 r7 s",
        ret=[(709.0, 0.8547249647390691), (1012.0, 0.5988142292490118)]),
    "episode_renderer_bench.timed": dict(
        log="c0 c1 s r0 c0 c0 r1 s r2 c1 c1 r3 s r4 c0 c0 r5 s r6 c1 c1 r7 s",
        ret=[(456.0, 1.1074561403508771), (708.5, 0.7127734650670431)]),
    "memory_train_bench.timed": dict(
        log="c0 s r0 c0 c0 r1 s",
        ret=153.0),
    "memory_policy_bench.time_ms": dict(
        log="c0 c0 c0 s r0 c0 c0 r1 s",
        ret=254.0),
    "rework_train_bench.mean_ms": dict(
        log="r0 c0 c0 r1 s",
        ret=52.0),
    "population_memory_agent_bench.per_call_us": dict(
        log="r0 c0 c0 r1 s",
        ret=52000.0),
}


def _us(t):
    return t * 1000.0


#: per parent loop: how the script that had it calls benchlib now, and the statistic it applies to the samples
NOW = {
    "linear_agent_bench.timed": lambda f: BL.median(BL.per_call(f, 2, 1)).tolist(),
    "population_bench.timed": lambda f: float(BL.median(BL.per_call(f[:1], 2, 1)[0])),
    "rework_agent_bench.rounds": lambda f: BL.median_spread(BL.per_block(f, 2, rounds=2, warmup=1)),
    "colony_stats_bench.blocks": lambda f: BL.median_spread(BL.per_block(f, 1, rounds=2, warmup=1)),
    "episode_renderer_bench.timed": lambda f: BL.median_spread(BL.per_block(f, 2, rounds=2, warmup=1, sync_blocks=True)),
    "memory_train_bench.timed": lambda f: float(BL.per_block(f[:1], 2, warmup=1)[0, 0]),
    "memory_policy_bench.time_ms": lambda f: float(BL.per_block(f[:1], 2, warmup=3)[0, 0]),
    "rework_train_bench.mean_ms": lambda f: float(BL.per_block(f[:1], 2, sync_blocks=True)[0, 0]),
    "population_memory_agent_bench.per_call_us": lambda f: float(_us(BL.per_block(f[:1], 2, sync_blocks=True))[0, 0]),
}


def test_every_parent_loop_has_a_trace():
    assert sorted(PARENT) == sorted(NOW) and len(PARENT) == 9


@pytest.mark.parametrize("label", sorted(NOW))
def test_loops_trace_and_values_equal_the_parents(label, monkeypatch):
    fake = FakeCuda(monkeypatch)
    got = NOW[label](fake.fns(2))
    want = PARENT[label]
    assert fake.compact() == want["log"]
    flat = lambda v: np.asarray(v, dtype=np.float64).ravel().tolist()  # noqa: E731
    assert flat(got) == flat(want["ret"])  # the same floats, not close ones


def test_per_block_takes_iters_per_fn_and_syncs_once_without_sync_blocks(monkeypatch):
    fake = FakeCuda(monkeypatch)
    t = BL.per_block(fake.fns(2), [1, 3], rounds=2)
    assert t.shape == (2, 2)
    assert fake.compact() == "r0 c0 r1 r2 c1 c1 c1 r3 r4 c0 r5 r6 c1 c1 c1 r7 s"
    # positions in the log, from 1: fn 0's pairs at (1, 3) and (9, 11), fn 1's at (4, 8) and (12, 16); fn 1's over its 3 calls
    assert t[0].tolist() == [103.0, 911.0] and t[1].tolist() == [408 / 3, 1216 / 3]


def test_warm_up_order_per_call_interleaves_per_block_goes_fn_by_fn(monkeypatch):
    fake = FakeCuda(monkeypatch)
    BL.per_call(fake.fns(2), 0, 2)
    assert fake.compact() == "c0 c1 c0 c1 s s"
    del fake.log[:]
    BL.per_block(fake.fns(2), 1, rounds=0, warmup=2)
    assert fake.compact() == "c0 c0 c1 c1 s s"


def test_statistics_on_a_2_by_5_array():
    t = np.array([[1.0, 2.0, 3.0, 4.0, 10.0], [5.0, 1.0, 3.0, 2.0, 4.0]])
    assert BL.median(t).tolist() == [3.0, 3.0]
    assert BL.median(t[:, :4]).tolist() == [2.5, 2.5]  # even length: the mean of the middle two
    # linear interpolation at q (n - 1): 10 % of 4 steps is 0.4 of the first gap, 90 % is 0.6 into the last
    np.testing.assert_allclose(BL.p50_p10_p90(t), [[3.0, 1.4, 7.6], [3.0, 1.4, 4.6]], rtol=1e-15)
    assert BL.abs_spread(t).tolist() == [9.0, 4.0]
    assert BL.rel_spread(t).tolist() == [3.0, 4.0 / 3.0]
    assert BL.median_spread(t) == [(3.0, 3.0), (3.0, 4.0 / 3.0)]
    assert BL.p50_p10_p90(t[0]).shape == (3,) and BL.median(t[0]) == 3.0  # a single row of samples


def test_members_are_the_three_copies():
    m = BL.members(5, 1e-4)
    assert list(m[0]) == ["epsilon", "discount", "learning_rate", "seed"]
    assert [x["learning_rate"] for x in m] == [1e-4 * (1 + p % 4) for p in range(5)]
    assert [x["discount"] for x in m] == [0.5 + 0.49 * p / 4 for p in range(5)] and [x["seed"] for x in m] == [1, 2, 3, 4, 5]
    assert BL.members(1, 1e-5, epsilon=None) == [dict(discount=0.5, learning_rate=1e-5, seed=1)]


@pytest.mark.parametrize("path", BENCHES, ids=[os.path.basename(p)[:-3] for p in BENCHES])
def test_every_bench_imports_without_a_gpu_and_has_a_main(path):
    assert len(BENCHES) == 19
    name = os.path.basename(path)[:-3]
    mod = __import__(name)
    assert os.path.samefile(mod.__file__, path)
    assert callable(mod.main)


def _imported_modules(source):
    names = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Import):
            names.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.module:
            names.add(node.module)
    return names


def test_no_stray_timing_events_and_no_bench_imports_a_bench():
    for path in sorted(glob.glob(os.path.join(PROFILES, "*.py"))):
        name = os.path.basename(path)
        with open(path) as f:
            source = f.read()
        if name not in ("benchlib.py", PRIVATE_LOOP):
            assert "enable_timing" not in source, name
        if name == PRIVATE_LOOP:
            assert "benchlib" in source and "private" in source, "the script that keeps its loop says so"
        for mod in _imported_modules(source):
            if mod.split(".")[-1].endswith("_bench"):
                assert (name[:-3], mod) == ALLOWED_IMPORT, "%s imports %s" % (name, mod)
