"""antsrl_amd/placement.py without a GPU: the tuner's decisions on recorded and hand-worked numbers, and the ORDER of what its
procedure does — allocations, handle re-creations, scratch episodes, measurements, releases — against a stand-in env, allocator
and device side that record every event and return scripted times.  The event lists are derived from the procedure as it stood inside
BatchedAntsEnv.tune_placement; they are also the short version of what the tuner does."""
import contextlib

import pytest
import torch

from antsrl_amd import placement
from antsrl_amd.placement import StateCandidate, Trial, pick_pair, pick_state, placement_levels_seen, report, spare_state_blocks

FRESH = [0.20761, 0.23375, 0.22291, 0.23091, 0.2008, 0.20152, 0.20208, 0.20301]      # a fresh process on a fast device
ONE_LEVEL = [0.23279, 0.23461, 0.23397, 0.23541, 0.23309, 0.23433, 0.23434, 0.23468]  # device 0xb6d3a6e8...: every trial slow


def test_placement_tuner_stopping_rule():
    """BatchedAntsEnv.tune_placement walks further into the device's memory until its trials have shown both placement levels
    (profiles/r05/two_colour.txt): the rule on recorded trial sets."""
    fresh, one_level = FRESH, ONE_LEVEL
    assert placement_levels_seen(fresh)
    assert not placement_levels_seen(one_level)
    assert not placement_levels_seen(one_level + [0.32247])          # an outlier is not a level
    assert placement_levels_seen(one_level + [0.32247, 0.2012])      # ... a buffer of another zone is
    assert not placement_levels_seen([0.0358, 0.0352, 0.0357, 0.0351])  # c2: no zone effect at all


def trials_of(perceive):
    return [Trial("pair %d" % k, None, None, p + 0.03, p, 0.034) for k, p in enumerate(perceive)]


def test_pick_pair():
    assert pick_pair(trials_of(FRESH)) == 4                       # 0.2008
    assert pick_pair(trials_of([0.2, 0.17, 0.19, 0.17])) == 1    # the first of equals


def cands_of(kinds, upd, prc):
    return [StateCandidate("state %d" % k, kind, None, p, u) for k, (kind, u, p) in enumerate(zip(kinds, upd, prc))]


def test_pick_state():
    """Worked by hand from the rule: candidate k is fast by `by` when upd[k] <= (1 - by) * upd[0] and upd[k] + prc[k] <
    upd[0] + prc[0]; a pieced block needs 3 %, a corner 5 %; a fast pieced block comes before any corner."""
    dpc, flat = ("default", "pieced", "corner"), [0.170] * 3
    assert pick_state(cands_of(dpc, [0.0340, 0.0320, 0.0318], flat)) == 1  # a block of its own comes before a corner
    assert pick_state(cands_of(dpc, [0.0340, 0.0338, 0.0322], flat)) == 2  # the corner's limit is 0.95 * 0.0340 = 0.0323
    assert pick_state(cands_of(dpc, [0.0340, 0.0338, 0.0325], flat)) == 0  # 0.0325 > 0.0323
    # the pieced block is fast, but k_perceive paid for it: the sums are 0.2050 against 0.2040
    assert pick_state(cands_of(dpc[:2], [0.0340, 0.0320], [0.170, 0.173])) == 0
    # two fast corners: the lower k_update_move time
    assert pick_state(cands_of(dpc + ("corner",), [0.0340, 0.0338, 0.0322, 0.0318], [0.170] * 4)) == 3
    assert pick_state(cands_of(dpc + ("corner",), [0.0340, 0.0338, 0.0318, 0.0322], [0.170] * 4)) == 2
    assert pick_state([StateCandidate("state torch (default)", "default", None)]) == 0  # (alone: not even measured)
    # the third device of DESIGN.md section 2: a default already on the fast level, nothing 3 % under it
    assert pick_state(cands_of(dpc + ("corner",), [0.0320, 0.0314, 0.0331, 0.0316], [0.170] * 4)) == 0


class Block:
    """What the tuner asks of a buffer: an address, a size, slices of it, zero_()."""
    next_ptr = 1 << 40

    def __init__(self, n, ptr=None):
        if ptr is None:
            ptr, Block.next_ptr = Block.next_ptr, Block.next_ptr + (1 << 40)
        self.n, self.ptr = n, ptr

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n

    def zero_(self):
        return self

    def __getitem__(self, s):
        assert s.start is None and s.stop <= self.n
        return Block(s.stop, self.ptr)


def test_spare_state_blocks():
    kept, small, a, b, c = Block(1000), Block(99), Block(1000), Block(100), Block(1000)
    trials = [Trial(label, ws, None, 0.2, 0.17, 0.03) for label, ws in (
        ("ws torch / out pieced", kept), ("ws small / out torch", small), ("ws pieced / out pieced", a),
        ("ws pieced / out torch", a), ("ws torch (walk 1: +48 GiB) / out pieced", b), ("ws last / out pieced", c))]
    spare = spare_state_blocks(trials, kept, 100, 3)
    assert [label for label, _ in spare] == ["state in spare record block (ws pieced)",
                                             "state in spare record block (ws torch (walk 1: +48 GiB))",
                                             "state in spare record block (ws last)"]
    assert [(blk.data_ptr(), blk.numel()) for _, blk in spare] == [(a.ptr, 100), (b.ptr, 100), (c.ptr, 100)]
    assert [blk.data_ptr() for _, blk in spare_state_blocks(trials, kept, 100, 2)] == [a.ptr, b.ptr]   # no more than `room`
    assert [blk.data_ptr() for _, blk in spare_state_blocks(trials, a, 100, 3)] == [kept.ptr, b.ptr, c.ptr]
    assert spare_state_blocks(trials, kept, 100, 0) == []


def test_report():
    trials = [Trial("ws torch / out pieced", None, None, 0.2312349, 0.2076149, 0.034),
              Trial("ws torch / out torch", None, None, 0.2598751, 0.2337551, 0.034)]
    cands = [StateCandidate("state torch (default)", "default", None, 0.1700049, 0.0340051),
             StateCandidate("state pieced", "pieced", None, 0.1699951, 0.0319949)]
    assert report(trials, 0, 2, cands, 1) == dict(
        ms_per_step=[0.23123, 0.25988], observation_kernel_ms=[0.20761, 0.23376], chosen=0,
        pairs=["ws torch / out pieced", "ws torch / out torch"], both_levels_seen=True, walk_steps=2,
        state_stage=dict(candidates=["state torch (default)", "state pieced"], update_move_kernel_ms=[0.03401, 0.03199],
                         observation_kernel_ms=[0.17, 0.17], chosen=1))
    assert list(report(trials, 0, 2, cands, 1)) == ["ms_per_step", "observation_kernel_ms", "chosen", "pairs", "both_levels_seen",
                                                    "walk_steps", "state_stage"]
    r = report(trials_of(ONE_LEVEL), 0, 0, [StateCandidate("state torch (default)", "default", None)], 0)
    assert r["both_levels_seen"] is False and r["both_levels_seen"] == placement_levels_seen(r["observation_kernel_ms"])
    assert r["state_stage"] == dict(candidates=["state torch (default)"], update_move_kernel_ms=[], observation_kernel_ms=[], chosen=0)
    r = report(trials_of(FRESH), 4, 0, cands, 0)
    assert r["both_levels_seen"] is True and r["both_levels_seen"] == placement_levels_seen(r["observation_kernel_ms"])


# ---------------------------------------------------------------------- the procedure's order of events
REC, OUT, STATE = 1000 << 20, 600 << 20, 100 << 20  # the env's byte counts: record block, output buffer, state block
WS, NEW_OUT, ST = REC + 256, OUT + 256, STATE + 256  # what the tuner draws (room to align); a RE-BOUND output buffer has OUT
GIB = 1 << 30


class StandInEnv:
    """The env as the tuner sees it.  Like BatchedAntsEnv it keeps `_out_flat` as the aligned OUT bytes of what it was
    handed — which is how the lists below tell a buffer bound again (OUT) from one drawn afresh (NEW_OUT)."""
    record_bytes, _out_total, state_bytes = REC, OUT, STATE

    def __init__(self, log, pieced=True):
        self.log, self._pieced, self._split = log, pieced, True
        self._ws, self._state, self._out_flat = Block(WS), Block(ST), Block(NEW_OUT)[:OUT]
        self._loaded, self.device = None, None

    def _make_handle(self, ws, state=None):
        self._ws, self._state = ws, state if state is not None else self._state
        self.log.append(("make_handle", ws.numel(), self._state.numel()))

    def _bind_outputs(self, flat):
        self.log.append(("bind_outputs", flat.numel()))
        self._out_flat = flat[:OUT]


class Allocator:
    """antsrl_amd/vmm.py, recording."""

    def __init__(self, log):
        self.log = log

    def empty_u8(self, n, dev):
        self.log.append(("empty_u8", n))
        return Block(n)

    def pieced_u8(self, n, dev):
        self.log.append(("pieced_u8", n))
        return Block(n)

    def trim(self):
        self.log.append(("trim",))


class ScriptedTuner(placement.Tuner):
    """The tuner with its device side replaced: allocations, episodes and measurements are logged, times come from a script
    of (k_perceive, k_update_move) pairs."""

    def __init__(self, script, pieced=True, **params):
        self.log, self.script = [], iter(script)
        params = dict(dict(age=150, steps=30, verbose=False, extra_outputs=4, walk_spacers=3, spacer_gib=24.0,
                           force_walk=False, state_stage=True), **params)  # (tune_placement's defaults)
        super().__init__(StandInEnv(self.log, pieced), **params)

    def device_side(self):
        return contextlib.nullcontext()

    def torch_u8(self, n):
        self.log.append(("torch_u8", n))
        return Block(n)

    def scratch_episode(self):
        self.log.append(("episode",))

    def measure(self, psteps=placement.PSTEPS):
        self.log.append(("measure", psteps))
        prc, upd = next(self.script)
        return prc + upd + 0.001, prc, upd


@pytest.fixture
def tuner(monkeypatch):
    """ScriptedTuner with the module's allocator and torch's free-memory and cache calls recording into its log."""
    def make(script, free_bytes=200 * GIB, **params):
        t = ScriptedTuner(script, **params)
        monkeypatch.setattr(placement, "vmm", Allocator(t.log))
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev: (free_bytes, 288 * GIB))
        monkeypatch.setattr(torch.cuda, "empty_cache", lambda: t.log.append(("empty_cache",)))
        return t
    return make


def stage_one_script(perceive):
    return [(p, 0.0340) for p in perceive]


EPISODE, MEASURE, MEASURE_STATE = ("episode",), ("measure", 8), ("measure", 24)
STAGE_ONE_PAIRS = [
    EPISODE, MEASURE,                                                       # the env's own pair: torch records, pieced outputs
    ("torch_u8", NEW_OUT), ("bind_outputs", NEW_OUT), MEASURE,              # ... against a torch output buffer
    ("empty_u8", WS), ("make_handle", WS, ST), EPISODE,                     # a pieced record block:
    ("bind_outputs", OUT), MEASURE,                                         # ... the env's own outputs, bound again
    ("torch_u8", NEW_OUT), ("bind_outputs", NEW_OUT), MEASURE,              # ... ANOTHER torch output buffer
]
EXTRA_DRAW = [("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), MEASURE]
EXTRA_DRAWS = [("make_handle", WS, ST), EPISODE] + 4 * EXTRA_DRAW           # back on the env's own records: four more pieced outputs
STATE_TRIAL = [("make_handle", WS, ST), ("bind_outputs", OUT), EPISODE, MEASURE_STATE]
KEEP = [("make_handle", WS, ST), ("bind_outputs", OUT)]                     # the handle once more, on what is kept


def walk_step(spacer, back_to_own_records):
    return ([("torch_u8", spacer), ("empty_u8", spacer)] + ([("make_handle", WS, ST)] if back_to_own_records else []) + [EPISODE]
            + [("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), MEASURE, ("torch_u8", NEW_OUT), ("bind_outputs", NEW_OUT), MEASURE]
            + [("torch_u8", WS), ("make_handle", WS, ST), EPISODE, ("bind_outputs", OUT), MEASURE])  # one more torch record block


def test_procedure_both_levels_at_once(tuner):
    """(a) The first eight trials show both levels: no walk.  Draw 2 wins; the state block goes to the pieced candidate."""
    t = tuner(stage_one_script(FRESH) + [(0.170, 0.0340), (0.170, 0.0320), (0.170, 0.0318)])
    times = t.run()
    assert t.log == [
        # stage one: the env's own pair — torch records, pieced outputs — and the same records against a torch output buffer
        ("episode",), ("measure", 8),
        ("torch_u8", NEW_OUT), ("bind_outputs", NEW_OUT), ("measure", 8),
        # a pieced record block: against the env's own outputs, bound again, and against ANOTHER torch output buffer
        ("empty_u8", WS), ("make_handle", WS, ST), ("episode",),
        ("bind_outputs", OUT), ("measure", 8),
        ("torch_u8", NEW_OUT), ("bind_outputs", NEW_OUT), ("measure", 8),
        # back on the env's own records: four more pieced output buffers
        ("make_handle", WS, ST), ("episode",),
        ("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), ("measure", 8),
        ("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), ("measure", 8),
        ("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), ("measure", 8),
        ("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), ("measure", 8),
        # stage two, on the chosen pair: the default state block, a pieced one, a corner of the pieced record block
        ("pieced_u8", ST),
        ("make_handle", WS, ST), ("bind_outputs", OUT), ("episode",), ("measure", 24),
        ("make_handle", WS, ST), ("bind_outputs", OUT), ("episode",), ("measure", 24),
        ("make_handle", WS, ST), ("bind_outputs", OUT), ("episode",), ("measure", 24),
        # the losers dropped, the handle once more on what is kept; no walk, so nothing to trim
        ("make_handle", WS, ST), ("bind_outputs", OUT), ("empty_cache",)]
    assert t.log == STAGE_ONE_PAIRS + EXTRA_DRAWS + [("pieced_u8", ST)] + 3 * STATE_TRIAL + KEEP + [("empty_cache",)]  # (the pieces below)
    r = t.env.placement_trials
    assert len(times) == 8 and r["chosen"] == 4 and r["walk_steps"] == 0 and r["both_levels_seen"]
    assert r["pairs"] == ["ws torch / out pieced", "ws torch / out torch", "ws pieced / out pieced", "ws pieced / out torch"] + [
        "ws torch / out pieced (draw %d)" % k for k in (2, 3, 4, 5)]
    assert r["state_stage"]["candidates"] == ["state torch (default)", "state pieced", "state in spare record block (ws pieced)"]
    assert r["state_stage"]["chosen"] == 1 and r["state_stage"]["update_move_kernel_ms"] == [0.034, 0.032, 0.0318]
    assert t.env._ws.numel() == WS and t.env._out_flat.numel() == OUT and t.env._loaded is None


def test_procedure_walks_until_the_second_level(tuner):
    """(b) One level through stage one; the walk's first step draws an output buffer of another zone: exactly one step."""
    t = tuner(stage_one_script(ONE_LEVEL + [0.2012, 0.2340, 0.2335]) + 4 * [(0.170, 0.0340)], walk_spacers=2)
    times = t.run()
    assert t.log == (STAGE_ONE_PAIRS + EXTRA_DRAWS
                     + walk_step(24 * GIB, back_to_own_records=False)   # (the extra draws left the handle on the env's own records)
                     + [("pieced_u8", ST)] + 4 * STATE_TRIAL   # default, pieced, corners of the pieced and the walk's record block
                     + KEEP + [("trim",), ("empty_cache",)])
    r = t.env.placement_trials
    assert len(times) == 11 and r["chosen"] == 8 and r["walk_steps"] == 1 and r["both_levels_seen"]
    assert r["pairs"][8:] == ["ws torch / out pieced (walk 1: +48 GiB)", "ws torch / out torch (walk 1: +48 GiB)",
                              "ws torch (walk 1: +48 GiB) / out pieced"]
    assert r["state_stage"]["candidates"][2:] == ["state in spare record block (ws pieced)",
                                                  "state in spare record block (ws torch (walk 1: +48 GiB))"]
    assert r["state_stage"]["chosen"] == 0


def test_procedure_forced_walk(tuner):
    """(c) force_walk=True, walk_spacers=2, extra_outputs=0 (tests/test_gpu_mem.py): 4 + 2 x 3 trials.  With memory short the
    spacer is a fifth of what is free; below 4 GiB the walk ends."""
    t = tuner(stage_one_script(FRESH + FRESH[:2]) + 4 * [(0.170, 0.0340)], free_bytes=30 * GIB,
                      force_walk=True, walk_spacers=2, extra_outputs=0, spacer_gib=8.0)
    times = t.run()
    assert t.log == (STAGE_ONE_PAIRS
                     + walk_step(6 * GIB, back_to_own_records=True) + walk_step(6 * GIB, back_to_own_records=True)
                     + [("pieced_u8", ST)] + 4 * STATE_TRIAL   # four candidates at the most: the second walk block is not tried
                     + KEEP + [("trim",), ("empty_cache",)])
    r = t.env.placement_trials
    assert len(times) == 4 + 2 * 3 and r["walk_steps"] == 2 and r["chosen"] == 4
    assert r["pairs"][4] == "ws torch / out pieced (walk 1: +12 GiB)" and r["pairs"][9] == "ws torch (walk 2: +24 GiB) / out pieced"
    assert len(r["state_stage"]["candidates"]) == 4
    short = tuner(stage_one_script(FRESH[:4]) + 3 * [(0.170, 0.0340)], free_bytes=19 * GIB, force_walk=True, extra_outputs=0)
    assert len(short.run()) == 4 and short.env.placement_trials["walk_steps"] == 0 and ("trim",) not in short.log


def test_procedure_without_pieced_memory(tuner):
    """(d) pieced_memory=False: the env's own outputs are torch memory and the OTHER kind is pieced; no extra draws, no walk
    — even with one level throughout."""
    t = tuner(stage_one_script(ONE_LEVEL[:4]) + 3 * [(0.170, 0.0340)], pieced=False)
    times = t.run()
    assert t.log == ([EPISODE, MEASURE,
                      ("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), MEASURE,
                      ("empty_u8", WS), ("make_handle", WS, ST), EPISODE,
                      ("bind_outputs", OUT), MEASURE,
                      ("empty_u8", NEW_OUT), ("bind_outputs", NEW_OUT), MEASURE]
                     + [("pieced_u8", ST)] + 3 * STATE_TRIAL
                     + KEEP + [("empty_cache",)])
    r = t.env.placement_trials
    assert len(times) == 4 and r["walk_steps"] == 0 and not r["both_levels_seen"]
    assert r["pairs"] == ["ws torch / out torch", "ws torch / out pieced", "ws pieced / out torch", "ws pieced / out pieced"]
