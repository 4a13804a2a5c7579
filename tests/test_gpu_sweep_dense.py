"""The explicit pheromone sweeps (csrc/antsrl_sweep.hip) on fields where every cell counts, at every strip and segment
seam: sweep_ref.CASES x {dense, near_cut, blocks, impulses} through BatchedAntsEnv with PHERO_EXPLICIT_SWEEP, the whole grid
against sweep_ref.sweep64 (float64, from the definition; test_sweep_ref_cpu.py ties it to the oracle and shows that every
defect of sweep_ref.DEFECTS fails the comparator on these very cases).

Gate: helpers.phero_close as it stands.  A cell outside it passes only if its error is inside the a-priori bound of the
kernel's own form, gamma_n |ref| with n fp32 roundings per output (sweep_ref.apriori_rtol: 2 S^2 general, 4 S separable,
1 at radius 0) — that is a finding about the comparator on dense fields, printed as FINDING with both shares; an error
outside the a-priori bound, a non-zero cell where the reference is zero or a zero where it is not (outside the cut's band)
fails.  At radius 1 and for the separable forms the a-priori bound is the narrower of the two and never decides.

Run with -s for the MEASURED lines: per kernel the largest relative error and where it sits.
"""
import numpy as np
import pytest

import helpers
import sweep_ref as S
from test_gpu_parity import _cpu, torch_mod  # noqa: F401  (the parity suite's fixture)

pytestmark = pytest.mark.gpu

MEASURED = {}   # kernel -> (largest relative error, where)
FINDINGS = []
DEFERRED = {}   # kernel -> does the library defer the update of its three-update case into the next step


def no_deposit_actions(cfg):
    rot = np.zeros((cfg.n_envs, cfg.n_ants), np.int8)
    return rot, (np.zeros((cfg.n_envs, cfg.n_ants), np.int8) if cfg.n_phero == 2 else None)


def _describe(plan, init, e, c, x, y, got, want):
    where = S.locate(plan, x, y, e)
    where["wall"] = bool(init["walls"][e, x, y])
    return "(env %d, channel %d, x %d, y %d) got %.9g want %.9g  %s" % (
        e, c, x, y, got, want, " ".join("%s=%s" % kv for kv in where.items()))


def _name_tap(plan, init, e, c, x, y):
    """impulses: the tap that produced output (x, y) — out[x, y] = F[a, b] * in[x - a + R, y - b + R]."""
    R = plan["R"]
    px, py = np.nonzero(init["phero"][e, c])
    near = [(x - p + R, y - q + R, p, q) for p, q in zip(px, py) if max(abs(x - p), abs(y - q)) <= R]
    return "".join(" tap F[%d,%d] of the impulse at (%d, %d)" % t for t in near) or " no impulse within R"


def check(case, plan, cfg, init, got, want, ctx, field=None):
    """The gate of the module docstring; records the kernel's largest relative error."""
    thr = cfg.phero_threshold
    got64 = got.astype(np.float64)
    ok = helpers.phero_close(got, want, threshold=thr)
    d = np.abs(got64 - want)
    band = S.in_cut_band(want, thr)
    nz = (want != 0) & ~band
    rel = np.where(nz, d / np.where(nz, want, 1.0), 0.0)
    if rel.size and rel.max() > MEASURED.get(case["kernel"], (-1.0, ""))[0]:
        i = np.unravel_index(np.argmax(rel), rel.shape)
        MEASURED[case["kernel"]] = (float(rel.max()), "%s %s %s" % (ctx, field or "", _describe(plan, init, *i, got64[i], want[i])))
    if ok.all():
        return
    rt = S.apriori_rtol(plan)
    bad = ~ok & ~(d <= rt * np.abs(want))
    if not bad.any():
        out = ~ok
        line = "FINDING %s %s %s: %d of %d cells (%.3g) outside helpers.phero_close, all inside the a-priori bound: " \
               "largest error %.3g |ref| = %.2f x PHERO_RTOL = %.2f x gamma_n (%.3g)" % (
                   case["kernel"], ctx, field or "", out.sum(), out.size, out.mean(), rel[out].max(),
                   rel[out].max() / helpers.PHERO_RTOL, rel[out].max() / rt, rt)
        FINDINGS.append(line)
        print(line)
        return
    cells = np.argwhere(bad)
    lines = []
    for e, c, x, y in cells[:8]:
        s = _describe(plan, init, e, c, x, y, got64[e, c, x, y], want[e, c, x, y])
        if field == "impulses":
            s += _name_tap(plan, init, e, c, x, y)
        lines.append(s)
    raise AssertionError("%s %s %s (%s): %d cells off (comparator and a-priori bound %.3g), wrong zeros %d, non-zero where the "
                         "reference is zero %d; first:\n  %s" % (
                             case["kernel"], ctx, field or "", case["name"], bad.sum(), rt, (bad & (got64 == 0)).sum(),
                             (bad & (want == 0)).sum(), "\n  ".join(lines)))


def _one_update(env, cfg, init):
    from antsrl_amd import config as cm
    env.reset(init)
    env.step(*no_deposit_actions(cfg), want_obs=False)
    env.update(None)
    return _cpu(env.read_state(cm.S_PHERO))


def _far_from_any_input(init, R):
    """[E, C, W, H] bool: cells farther than R (in either axis) from every non-zero, non-wall input cell."""
    live = (init["phero"] != 0) & (init["walls"][:, None] == 0)
    E, C, W, H = live.shape
    pad = np.zeros((E, C, W + 2 * R, H + 2 * R), bool)
    pad[:, :, R:R + W, R:R + H] = live
    near = np.zeros_like(live)
    for a in range(2 * R + 1):
        for b in range(2 * R + 1):
            near |= pad[:, :, a:a + W, b:b + H]
    return ~near


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_one_update_on_every_field(torch_mod, case):
    from antsrl_amd.batched import BatchedAntsEnv
    cfg = S.make_case_cfg(case)
    plan = S.sweep_plan(cfg)
    env = BatchedAntsEnv(cfg)
    for field in S.FIELDS:
        if case.get("huge") and field != "dense":
            continue  # (the one 17 MB grid is there for the scalar kernel's second grid-stride pass)
        init = S.make_init(case, cfg, field)
        got = _one_update(env, cfg, init)
        want = S.reference(cfg, init)
        check(case, plan, cfg, init, got, want, case["name"], field)
        if field == "blocks":
            far = _far_from_any_input(init, plan["R"])
            assert far.any()
            bits = got.view(np.uint32)[far]
            assert not bits.any(), "%s blocks: %d cells farther than R from every non-zero input are not +0.0; first: %s" % (
                case["name"], np.count_nonzero(bits),
                _describe(plan, init, *np.argwhere(far & (got.view(np.uint32) != 0))[0], 0, 0))


_MULTI = [c for c in S.CASES if c.get("multi")]
_MULTI_IDS = [c["name"].replace(" ", "_") for c in _MULTI]


@pytest.mark.parametrize("field", ["dense", "near_cut"])
@pytest.mark.parametrize("case", _MULTI, ids=_MULTI_IDS)
def test_three_updates_immediate_and_deferred(torch_mod, case, field):
    """Handle A reads the grid after every update (each update runs at once, on both buffers of the ping-pong in turn)
    and is compared at every step; handle B reads nothing in between (where the library can, the update waits for the
    next step and the sweep follows k_update_move) and is compared at the end.  The two agree in every bit."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    cfg = S.make_case_cfg(case)
    plan = S.sweep_plan(cfg)
    _, init, refs = S.multi_inputs(case, field)
    a, b = BatchedAntsEnv(cfg), BatchedAntsEnv(cfg)
    DEFERRED[case["kernel"]] = a.query(cm.Q_DEFERRED_UPDATE)
    a.reset(init)
    b.reset(init)
    act = no_deposit_actions(cfg)
    for t in range(S.MULTI_STEPS):
        a.step(*act, want_obs=False)
        a.update(None)
        got = _cpu(a.read_state(cm.S_PHERO))
        check(case, plan, cfg, init, got, refs[t], "%s update %d" % (case["name"], t + 1), field)
        b.step(*act, want_obs=False)
        b.update(None)
    end = b.read_state(cm.S_PHERO)
    assert torch_mod.equal(a.read_state(cm.S_PHERO), end), "%s %s: a read between the updates changes the grid" % (case["name"], field)
    check(case, plan, cfg, init, _cpu(end), refs[-1], "%s no read in between" % case["name"], field)


@pytest.mark.parametrize("case", _MULTI, ids=_MULTI_IDS)
def test_deposits_on_a_dense_field_vs_oracle(torch_mod, case):
    """64 ants deposit 256 per step on top of the dense field (sweep_ref.deposit_inputs), so that deposits land on non-zero
    cells beside the seams and are swept at the next update: two steps against the oracle.  No cell of the oracle's grid
    lies inside the cut's band after either update (test_sweep_ref_cpu.py asserts it)."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from oracle.oracle import Oracle
    cfg, init, act, steps = S.deposit_inputs(case)
    plan = S.sweep_plan(cfg)
    env, orc = BatchedAntsEnv(cfg), Oracle(cfg, init, n_threads=4)
    env.reset(init)
    if act is not None:
        env.set_activation(act)
        orc.set_activation(act)
    for t, (rot, ph, jit) in enumerate(steps):
        env.step(rot, ph, want_obs=False)
        orc.step(rot, ph, want_obs=False)
        env.update(jit)
        orc.update(jit)
        check(case, plan, cfg, init, _cpu(env.read_state(cm.S_PHERO)), orc.phero, "%s deposits, update %d" % (case["name"], t + 1))
    np.testing.assert_array_equal(np.floor(_cpu(env.read_state(cm.S_ANTS_XYT))[..., :2]), np.floor(orc.ants_xyt[..., :2]))


@pytest.mark.parametrize("case", _MULTI, ids=_MULTI_IDS)
def test_environment_1_alone_gives_the_same_bits(torch_mod, case):
    from antsrl_amd.batched import BatchedAntsEnv
    cfg = S.make_case_cfg(case)
    init = S.make_init(case, cfg, "dense")
    batch = _one_update(BatchedAntsEnv(cfg), cfg, init)
    cfg1 = S.make_case_cfg(case, E=1, env_id_base=1)
    alone = _one_update(BatchedAntsEnv(cfg1), cfg1, {k: (None if v is None else v[1:2]) for k, v in init.items()})
    np.testing.assert_array_equal(batch[1].view(np.uint32), alone[0].view(np.uint32), err_msg=case["name"])


def test_measured_lines(torch_mod):
    """Last in the file: what the tests above measured (needs them to have run in this process)."""
    print()
    for k in sorted(MEASURED):
        print("MEASURED %-24s largest relative error %.3g = %.2f x PHERO_RTOL at %s" % (
            k, MEASURED[k][0], MEASURED[k][0] / helpers.PHERO_RTOL, MEASURED[k][1]))
    print("FINDINGS: %d" % len(FINDINGS))
    print("DEFERRED UPDATE in the three-update cases: %s; at once: %s" % (
        " ".join(k for k in sorted(DEFERRED) if DEFERRED[k]) or "-", " ".join(k for k in sorted(DEFERRED) if not DEFERRED[k]) or "-"))
    if len(MEASURED) > 1:  # (a run of the whole file)
        assert set(MEASURED) == set(S.FAMILIES), set(S.FAMILIES) ^ set(MEASURED)
