"""BatchedAntsEnv.tune_placement's tuner: which buffers the env keeps, decided by timing.

The DECISIONS are pure functions over records of what was measured — `placement_levels_seen` (walk on?), `pick_pair`,
`spare_state_blocks`, `pick_state`, `report` — and run on recorded numbers without a GPU (tests/test_placement_cpu.py).
The PROCEDURE is `Tuner`: it draws the buffers, steps the scratch episodes and measures, against the few things it needs
of the env (`_make_handle`, `_bind_outputs`, `generate`, `step_update`, `set_timing_events`, the byte counts) and the two
allocators (torch.empty, antsrl_amd/vmm.py).  Which zone an allocator draws from depends on what was allocated and freed
before: the ORDER of the procedure's allocations, handle re-creations and releases is part of what it does."""
import contextlib
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import config as cfgmod
from . import vmm

#: one stage-one measurement: a (record block `ws`, output buffer `out`) pair stepped at one point of a scratch episode
Trial = namedtuple("Trial", "label ws out ms_per_step perceive_ms update_ms")
#: one stage-two candidate for the state block; kind: "default" (the env's own), "pieced" (a block of its own) or "corner"
#: (of a spare record block); the times are None until it has been measured
StateCandidate = namedtuple("StateCandidate", "label kind block perceive_ms update_ms", defaults=(None, None))

OUTLIER = 1.25       # a trial this far above the fastest is not a level (a first touch, a profiler's hiccup)
LEVEL_SPREAD = 1.06  # k_perceive's levels: 15-18 % apart at c3 / c4 / c5, 3-4 % at c2-sized batches — which then walk
# The two levels of k_update_move lie 6 % apart (0.0340 / 0.0320 ms at c3); a candidate replaces the default only when it is
# faster by half of that — anything less is one level, measured twice — and k_perceive, the larger kernel, has not paid for it.
PIECED_GAIN = 0.03
# A block of its own comes before a corner of a spare record block, whose other bytes (1 GB at c3) would stay allocated for
# nothing: a corner is kept only where no block of its own reaches the fast level, and only for 5 % (corners measure 2-4 %
# under a default that is already on the fast level: profiles/r06).
CORNER_GAIN = 0.05
PSTEPS = 8           # steps under the library's timing hook per stage-one trial
PSTEPS_STATE = 24    # (stage two looks for 6 % on a kernel a fifth as long: more samples)
MAX_STATE_CANDIDATES = 4


def placement_levels_seen(times) -> bool:
    """tune_placement's stopping rule: have the trials — the observation kernel's times — shown BOTH placement levels (15 %
    apart at c3)?  A spread of 6 % or more among the trials — not counting a trial far above everything else, which is not a level (a
    first touch, a profiler's hiccup: 0.32 ms among 0.233s on a device whose every buffer sat on the slow level)."""
    ok = [t for t in times if t < OUTLIER * min(times)]
    return max(ok) >= LEVEL_SPREAD * min(ok)


def pick_pair(trials) -> int:
    """The pair with the fastest observation kernel (the step time around it carries the timing hook's own stalls); the
    first of equals."""
    return min(range(len(trials)), key=lambda k: trials[k].perceive_ms)


def spare_state_blocks(trials, kept_ws, n_state, room):
    """[(label, block)]: a corner of `n_state` bytes of each record block stage one drew and did not keep (other zones,
    already paid for), in trial order, every block once, `room` of them at most."""
    seen, spare = {kept_ws.data_ptr()}, []
    for t in trials:
        if t.ws.data_ptr() not in seen and t.ws.numel() >= n_state and len(spare) < room:
            seen.add(t.ws.data_ptr())
            spare.append(("state in spare record block (%s)" % t.label.split(" / ")[0], t.ws[:n_state]))
    return spare


def pick_state(cands) -> int:
    """The state block to keep: cands[0] is the default; the fastest pieced block that is fast by PIECED_GAIN, else the
    fastest corner that is fast by CORNER_GAIN, else the default (as when it stands alone, unmeasured)."""
    upd, prc = [c.update_ms for c in cands], [c.perceive_ms for c in cands]

    def fast(k, by):
        return upd[k] <= (1.0 - by) * upd[0] and upd[k] + prc[k] < upd[0] + prc[0]
    own = [k for k in range(1, len(cands)) if cands[k].kind == "pieced" and fast(k, PIECED_GAIN)]
    corners = [k for k in range(1, len(cands)) if cands[k].kind == "corner" and fast(k, CORNER_GAIN)]
    return min(own or corners, key=upd.__getitem__) if own or corners else 0


def report(trials, chosen, walk_steps, cands, state_chosen) -> dict:
    """`placement_trials` (bench.py prints it whole).  A lone default state candidate was not measured: no times."""
    prc = [t.perceive_ms for t in trials]
    measured = [c for c in cands if c.update_ms is not None]
    return dict(ms_per_step=[round(t.ms_per_step, 5) for t in trials], observation_kernel_ms=[round(t, 5) for t in prc],
                chosen=chosen, pairs=[t.label for t in trials], both_levels_seen=bool(placement_levels_seen(prc)),
                walk_steps=walk_steps,
                state_stage=dict(candidates=[c.label for c in cands], update_move_kernel_ms=[round(c.update_ms, 5) for c in measured],
                                 observation_kernel_ms=[round(c.perceive_ms, 5) for c in measured], chosen=state_chosen))


class Tuner:
    """One run of tune_placement on `env` (its docstring says what and why).  `run` is the procedure, in three stages; the
    methods before it are its device side: actions and events, scratch episodes, measurements."""

    def __init__(self, env, age, steps, verbose, extra_outputs, walk_spacers, spacer_gib, force_walk, state_stage):
        self.env, self.dev, self.age, self.steps, self.verbose = env, env.device, age, steps, verbose
        self.extra_outputs, self.walk_spacers, self.spacer_gib = int(extra_outputs), int(walk_spacers), spacer_gib
        self.force_walk, self.state_stage = force_walk, state_stage
        self.n_ws, self.n_out, self.n_state = env.record_bytes + 256, env._out_total + 256, env.state_bytes + 256

    @contextlib.contextmanager
    def device_side(self):
        """The env's device current, four steps of uniform random actions, and the events the measurements read."""
        c, dev = self.env.cfg, self.dev
        with torch.cuda.device(dev):
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            self.rot = torch.randint(-1, 2, (4, c.n_envs, c.n_ants), generator=g, device=dev, dtype=torch.int8)
            self.ph = torch.randint(0, 3, (4, c.n_envs, c.n_ants), generator=g, device=dev, dtype=torch.int8) if c.n_phero == 2 else [None] * 4
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.evs = _lib.HipEvents(cfgmod.TIMING_EVENTS * PSTEPS_STATE)
            yield
            self.evs.destroy()

    def torch_u8(self, n):
        return torch.empty(n, dtype=torch.uint8, device=self.dev)

    def new_out(self, pieced):
        return (vmm.empty_u8(self.n_out, self.dev) if pieced else self.torch_u8(self.n_out)).zero_()

    def step(self, t):
        self.env.step_update(self.rot[t % 4], self.ph[t % 4], None)

    def scratch_episode(self):
        self.env.generate(cfgmod.make_gen(), episode_seed=0x7A11)
        for t in range(self.age):
            self.step(t)

    def measure(self, psteps=PSTEPS):
        """-> (ms per step over `steps` steps, k_perceive's ms, k_update_move's ms: the means of `psteps` further steps)."""
        NEV, evs = cfgmod.TIMING_EVENTS, self.evs
        for t in range(4):
            self.step(t)
        self.e0.record()
        for t in range(self.steps):
            self.step(t)
        self.e1.record()
        for t in range(psteps):  # (then a few steps with the library's timing hook: k_perceive by HIP events)
            self.env.set_timing_events([evs.ev[NEV * t + i].value for i in range(NEV)])
            self.step(t)
        torch.cuda.current_stream(self.dev).synchronize()
        # the observation kernel alone (events [2]..[3]): what the zones act on (the levels are read off THIS); and
        # k_update_move alone (events [1]..[2]): what the second stage reads
        prc = float(np.mean([evs.elapsed_ms(NEV * t + 2, NEV * t + 3) for t in range(psteps)]))
        upd = float(np.mean([evs.elapsed_ms(NEV * t + 1, NEV * t + 2) for t in range(psteps)]))
        return self.e0.elapsed_time(self.e1) / self.steps, prc, upd

    def trial(self, label, out=None):
        """One stage-one measurement where the scratch episode stands, on the output buffer `out` (None: the one bound)."""
        if out is not None:
            self.env._bind_outputs(out)
        return Trial(label, self.env._ws, self.env._out_flat, *self.measure())

    # ------------------------------------------------------------------ the procedure
    def stage_one(self, own_ws, own_out):
        """The env's own pair first (workspace torch.empty, outputs pieced unless pieced_memory=False), then the other
        three — the other kind of output buffer drawn AFRESH under each workspace — then `extra_outputs` more draws of
        the default kind."""
        env, trials = self.env, []
        own, other = ("pieced", "torch") if env._pieced else ("torch", "pieced")
        for ws_kind in ("torch", "pieced"):
            if ws_kind == "pieced":
                env._make_handle(vmm.empty_u8(self.n_ws, self.dev))  # (the env's own record block is torch.empty memory)
            self.scratch_episode()
            trials.append(self.trial("ws %s / out %s" % (ws_kind, own), own_out if ws_kind == "pieced" else None))
            trials.append(self.trial("ws %s / out %s" % (ws_kind, other), self.new_out(other == "pieced")))
        if self.extra_outputs > 0 and env._pieced:
            env._make_handle(own_ws)
            self.scratch_episode()
            for k in range(self.extra_outputs):
                trials.append(self.trial("ws torch / out pieced (draw %d)" % (k + 2), self.new_out(True)))
        return trials

    def walk(self, trials, own_ws, own_out):
        """Both levels seen?  If not, walk further into the device's memory until a buffer of another zone turns up.
        Appends to `trials`; -> (the spacers, to be held until the losing buffers go; the steps walked)."""
        env, spacers, walked = self.env, [], 0
        while env._pieced and walked < self.walk_spacers and (
                self.force_walk or not placement_levels_seen([t.perceive_ms for t in trials])):
            # one step of the walk: a spacer from EACH allocator (hipMalloc and the virtual-memory one draw from
            # different ends of the device's memory: profiles/r05/two_colour.txt), then one more output buffer of each
            # kind against the env's own workspace, and the env's own output buffer against one more torch workspace
            want = int(min(self.spacer_gib * 2 ** 30, torch.cuda.mem_get_info(self.dev)[0] / 5))
            if want < (4 << 30):
                break
            try:
                spacers.append(self.torch_u8(want))
                spacers.append(vmm.empty_u8(want, self.dev))
            except (RuntimeError, _lib.AntsrlError):
                break
            walked += 1
            where = "walk %d: +%.0f GiB" % (walked, sum(x.numel() for x in spacers) / 2 ** 30)
            if env._ws.data_ptr() != own_ws.data_ptr():
                env._make_handle(own_ws)
            self.scratch_episode()
            for kind in ("pieced", "torch"):
                trials.append(self.trial("ws torch / out %s (%s)" % (kind, where), self.new_out(kind == "pieced")))
            env._make_handle(self.torch_u8(self.n_ws))
            self.scratch_episode()
            trials.append(self.trial("ws torch (%s) / out pieced" % where, own_out))
        return spacers, walked

    def stage_two(self, trials, ws, out, own_state):
        """The pair (ws, out) stays; the STATE block — what k_update_move streams while it scatters into the records — is
        tried on the env's own torch.empty block, a pieced one, and a corner of the record blocks the first stage drew
        and did not keep; k_update_move's own time decides.  The default is measured again, at
        PSTEPS_STATE steps like its rivals.  -> the candidates, measured unless the default stands alone."""
        env, cands = self.env, [StateCandidate("state torch (default)", "default", own_state)]
        if self.state_stage and env._split:
            with contextlib.suppress(_lib.AntsrlError):
                cands.append(StateCandidate("state pieced", "pieced", vmm.pieced_u8(self.n_state, self.dev)))
            cands += [StateCandidate(label, "corner", block) for label, block in
                      spare_state_blocks(trials, ws, self.n_state, MAX_STATE_CANDIDATES - len(cands))]
        for k, c in enumerate(cands) if len(cands) > 1 else []:
            env._make_handle(ws, c.block)
            env._bind_outputs(out)
            self.scratch_episode()
            _, prc, upd = self.measure(PSTEPS_STATE)
            cands[k] = c._replace(perceive_ms=prc, update_ms=upd)
        return cands

    def run(self):
        """-> the stage-one ms/step figures; leaves the env on the kept buffers with `placement_trials` written."""
        env = self.env
        with self.device_side():
            own_ws, own_out, own_state = env._ws, env._out_flat, env._state
            trials = self.stage_one(own_ws, own_out)
            spacers, walked = self.walk(trials, own_ws, own_out)
            best, times = pick_pair(trials), [t.ms_per_step for t in trials]
            if self.verbose:
                print("tune_placement: ms/step per (workspace, outputs) pair %s -> %d" % (["%.4f" % t for t in times], best))
            ws, out = trials[best].ws, trials[best].out
            cands = self.stage_two(trials, ws, out, own_state)
            s_best = pick_state(cands)
            state = cands[s_best].block
            env.placement_trials = report(trials, best, walked, cands, s_best)
            del trials, spacers, cands  # the losing buffers go BEFORE the handle is re-created on the kept ones
            if ws.data_ptr() != env._ws.data_ptr() or (state is not None and state.data_ptr() != env._state.data_ptr()):
                env._make_handle(ws, state)
            env._bind_outputs(out)
            if walked:  # (the walk's spacers and losing buffers: torch's go back to the driver, the pool's are unmapped — their
                vmm.trim()  # ranges retired, never re-used; without a walk the few losing buffers simply stay pooled)
            torch.cuda.empty_cache()
            env._out_flat.zero_()
        env._loaded = None  # (the scratch episodes were the tuner's own: the handle is as new)
        return times
