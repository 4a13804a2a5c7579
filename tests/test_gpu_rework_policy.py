"""The rework agent's net on the device (ReworkPolicy: antsrl_rework_collapse, antsrl_policy_rework) against the comparators
of tests/rework_policy_ref.py, which tests/test_rework_policy_fixture.py pins to the reference's own classes.

  collapse   the collapsed buffer equals `collapse64` in every bit.
  accuracy   |q_dev - q64| <= 4 e_ref, q64 the float64 layered forward and e_ref the reference's own fp32 error on the
             same inputs (the fixture's, or e_ref() on the values the kernel was given).  The margin of 4 covers a
             summation order that differs from torch's blocked one and stays three orders of magnitude below what bf16
             operands would give; the measured ratio is printed (run with -s) and recorded in DESIGN §7.14.
  actions    the actions are the first argmax of the kernel's own q, and equal the float64 argmax (for the fixture also the
             reference's recorded actions) on every row whose float64 top-two gap exceeds 8 e_ref; at most 1 % of a
             test's rows are left out, and among the compared rows every action of a head with two or more outputs
             occurs.  Two exceptions to the last clause, both by construction: the fixture's `init` model takes one
             action on every row (its q is dominated by the biases: the reason the fixture has `spread`), and a batch of
             one row holds one action.
Bit comparisons are agent_harness.same_bits'.  The GPU tests read only the fixture, never the reference's checkout."""
import functools

import numpy as np
import pytest

import rework_policy_ref as R
from agent_harness import make_env, same_bits

pytestmark = pytest.mark.gpu

SHAPES = ((9, 3, 3), (147, 1, 1), (147, 5, 2), (294, 5, 2), (1022, 3, 3))  # (F, n_rot, n_ph); the last has D = 1024, the limit
BATCHES = (1, 31, 33, 255, 257, 2049)  # one row; around the 32 rows a workgroup takes per pass; a ragged last pass
SEED = 1
FORMATS = ("float32", "bfloat16")


def _policy(sd, F):
    from antsrl_amd.policy import ReworkPolicy
    pol = ReworkPolicy(F, "cuda", seed=99)
    pol.load_state_dict(sd)
    return pol


def _act(pol, obs, ast, fmt, logits=True):
    """obs [M, F] and ast [M, 2] (CPU, float32) through pol.act in observation format `fmt` -> (q or None, rot, ph), CPU."""
    import torch
    M, F = obs.shape
    o = obs.to("cuda", getattr(torch, fmt)).view(M, 1, 1, F).contiguous()
    q = torch.empty((M, pol.n_rot + pol.n_ph), dtype=torch.float32, device="cuda") if logits else None
    rot, ph = pol.act(o, ast.to("cuda"), logits=q)
    assert rot.shape == ph.shape == (M,) and rot.dtype == ph.dtype == torch.int8
    return (q.cpu() if logits else None), rot.cpu().clone(), ph.cpu().clone()


def _bf16(obs):
    import torch
    return obs.to(torch.bfloat16).to(torch.float32)


def _check_accuracy(what, q, q64, e):
    """(b): |q_dev - q64| <= 4 e_ref; returns the measured ratio."""
    ratio = float((q.double() - q64).abs().max()) / e
    print("%s: max |q_dev - q64| = %.3g = %.3f e_ref (e_ref %.3g)" % (what, ratio * e, ratio, e))
    assert ratio <= 4.0, (what, ratio, e)
    return ratio


def _check_actions(what, q, rot, ph, q64, e, n_rot, recorded=None, coverage=True):
    """(c)."""
    import torch
    n_ph = q.shape[1] - n_rot
    own_rot, own_ph = R.actions(q, n_rot)
    assert torch.equal(rot.long(), own_rot) and torch.equal(ph.long(), own_ph), what  # first argmax of its own q
    keep = R.top2_gap(q64, n_rot) > 8 * e
    left_out = int((~keep).sum())
    print("%s: %d of %d rows within 8 e_ref of a tie" % (what, left_out, len(keep)))
    assert left_out <= 0.01 * len(keep), (what, left_out, len(keep))
    want_rot, want_ph = R.actions(q64, n_rot)
    assert torch.equal(rot.long()[keep], want_rot[keep]) and torch.equal(ph.long()[keep], want_ph[keep]), what
    if recorded is not None:
        assert torch.equal(rot[keep], recorded[0][keep]) and torch.equal(ph[keep], recorded[1][keep]), what
    if coverage:
        for a, n in ((want_rot[keep], n_rot), (want_ph[keep], n_ph)):
            assert n < 2 or len(set(a.tolist())) == n, (what, sorted(set(a.tolist())), n)


# ---- the inputs, built once ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(model):
    """(sd, policy, obs [T * 64, 294], agent_state, recorded actions, recorded q64, recorded e_ref per step [T])."""
    import torch
    sd, rec = R.load_model(model)
    T = rec["obs"].shape[0]
    return dict(sd=sd, pol=_policy(sd, 294), T=T, obs=torch.from_numpy(rec["obs"]).reshape(T * 64, 294),
                ast=torch.from_numpy(rec["agent_state"]).reshape(T * 64, 2),
                rot=torch.from_numpy(rec["rotation"]).reshape(-1), ph=torch.from_numpy(rec["pheromone"]).reshape(-1),
                q64=torch.from_numpy(rec["q64"]).reshape(T * 64, 6), e_ref=rec["e_ref"])


@functools.lru_cache(maxsize=None)
def _synthetic(shape):
    """The shape's 2049 synthetic rows (a smaller batch is their head), its policy, and per row the reference's fp32
    error and the float64 q."""
    F, n_rot, n_ph = shape
    sd, obs, ast = R.synthetic(F, n_rot, n_ph, max(BATCHES), SEED)
    err, q64 = R.row_errors(sd, obs, ast)
    return dict(sd=sd, pol=_policy(sd, F), obs=obs, ast=ast, err=err, q64=q64)


# ---- (a) the collapse, bit for bit --------------------------------------------------------------------------------------
def _check_collapse(pol, sd):
    wc, bc = R.collapse64(sd)
    assert same_bits(pol.collapsed_weight.cpu(), wc), "Wc: %d of %d elements differ" % (
        int((pol.collapsed_weight.cpu() != wc).sum()), wc.numel())
    assert same_bits(pol.collapsed_bias.cpu(), bc)


@pytest.mark.parametrize("model", R.MODELS)
def test_collapse_of_the_fixture_models_bit_for_bit(model):
    f = _fixture(model)
    assert f["pol"].collapsed_weight.shape == (6, 296) and f["pol"].collapsed_bias.shape == (6,)
    _check_collapse(f["pol"], f["sd"])


@pytest.mark.parametrize("shape", SHAPES)
def test_collapse_of_the_synthetic_shapes_bit_for_bit(shape):
    s = _synthetic(shape)
    _check_collapse(s["pol"], s["sd"])
    # and a second collapse of the same weights gives the same bits
    first = s["pol"].collapsed.clone()
    s["pol"].load_state_dict(s["sd"])
    assert same_bits(first.cpu(), s["pol"].collapsed.cpu())


# ---- (b), (c) on the fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("model", R.MODELS)
def test_fixture_steps_accuracy_and_actions(model, fmt):
    import torch
    f = _fixture(model)
    obs = f["obs"] if fmt == "float32" else _bf16(f["obs"])
    q, rot, ph = _act(f["pol"], obs, f["ast"], fmt)
    exact = torch.equal(obs, f["obs"])  # bfloat16: the recorded float64 q and actions hold only where nothing was rounded
    if exact:
        q64, e_steps = f["q64"], f["e_ref"]
    else:
        err, q64 = R.row_errors(f["sd"], obs, f["ast"])
        e_steps = [float(err[t * 64:(t + 1) * 64].max()) for t in range(f["T"])]
    worst = 0.0
    for t in range(f["T"]):
        rows = slice(t * 64, (t + 1) * 64)
        worst = max(worst, _check_accuracy("%s %s step %d" % (model, fmt, t), q[rows], q64[rows], float(e_steps[t])))
    print("%s %s: largest ratio %.3f" % (model, fmt, worst))
    _check_actions("%s %s" % (model, fmt), q, rot, ph, q64, float(max(e_steps)), 3,
                   recorded=(f["rot"], f["ph"]) if exact else None, coverage=model == "spread")


# ---- (d) shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_accuracy_and_actions(shape, M, fmt):
    s = _synthetic(shape)
    q, rot, ph = _act(s["pol"], s["obs"][:M], s["ast"][:M], fmt)  # (the synthetic values are bfloat16 values already)
    e = float(s["err"][:M].max())
    what = "F %d heads %d+%d M %d %s" % (shape + (M, fmt))
    _check_accuracy(what, q, s["q64"][:M], e)
    _check_actions(what, q, rot, ph, s["q64"][:M], e, shape[1], coverage=M > 1)


# ---- (e) a row depends on itself only ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((294, 5, 2), (147, 5, 2)))
def test_a_row_depends_on_itself_only(shape):
    import torch
    s = _synthetic(shape)
    obs, ast, pol = s["obs"][:257], s["ast"][:257], s["pol"]
    for fmt in FORMATS:
        q, rot, ph = _act(pol, obs, ast, fmt)
        q2, rot2, ph2 = _act(pol, obs, ast, fmt)  # a second launch
        assert same_bits(q, q2) and torch.equal(rot, rot2) and torch.equal(ph, ph2), fmt
        qa, rota, pha = _act(pol, obs[:31], ast[:31], fmt)  # the first 31 rows alone
        assert same_bits(qa, q[:31]) and torch.equal(rota, rot[:31]) and torch.equal(pha, ph[:31]), fmt
        back = torch.cat([torch.arange(31, 257), torch.arange(31)])  # ... and at the end of the batch
        qb, rotb, phb = _act(pol, obs[back], ast[back], fmt)
        assert same_bits(qb[-31:], q[:31]) and torch.equal(rotb[-31:], rot[:31]) and torch.equal(phb[-31:], ph[:31]), fmt
        assert same_bits(qb[:-31], q[31:]), fmt
        if fmt == "float32":
            q32, rot32, ph32 = q, rot, ph
    assert same_bits(q, q32) and torch.equal(rot, rot32) and torch.equal(ph, ph32)  # bfloat16 against float32


def test_rows_beyond_two_to_the_31_elements():
    """Element indices past 2^31 and byte offsets past 2^32: the last rows of 7.4 million bfloat16 rows of 294 (4.4 GB,
    zeros in front) get the bits they get alone."""
    import torch
    s = _synthetic((294, 5, 2))
    M, n = 7_400_000, 33
    assert (M - n) * 294 > 2 ** 31
    obs = torch.zeros((M, 1, 1, 294), dtype=torch.bfloat16, device="cuda")
    ast = torch.zeros((M, 2), dtype=torch.float32, device="cuda")
    obs[-n:] = s["obs"][:n].to("cuda", torch.bfloat16).view(n, 1, 1, 294)
    ast[-n:] = s["ast"][:n].to("cuda")
    q = torch.empty((M, 7), dtype=torch.float32, device="cuda")
    rot, ph = s["pol"].act(obs, ast, logits=q)
    got = q[-n:].cpu(), rot[-n:].cpu().clone(), ph[-n:].cpu().clone()
    zero_row = q[0].cpu().clone(), q[M - n - 1].cpu().clone()
    del obs, ast, q
    qa, rota, pha = _act(s["pol"], s["obs"][:n], s["ast"][:n], "bfloat16")
    assert same_bits(got[0], qa) and torch.equal(got[1], rota) and torch.equal(got[2], pha)
    assert same_bits(zero_row[0], s["pol"].collapsed_bias.cpu()) and same_bits(zero_row[1], zero_row[0])  # x = 0: q = bc


# ---- (f) nothing else is written -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_nothing_else_is_written(fmt):
    import torch
    s = _synthetic((147, 5, 2))
    pol, M, G = s["pol"], 257, 64
    obs = s["obs"][:M].to("cuda", getattr(torch, fmt)).view(M, 1, 1, 147).contiguous()
    ast = s["ast"][:M].to("cuda")
    bufs = {k: torch.full((G + n + G,), 0xFF, dtype=torch.uint8, device="cuda") for k, n in
            (("rot", M), ("ph", M), ("q", 4 * 7 * M))}
    keep = pol._rot, pol._ph
    try:
        pol._rot, pol._ph = bufs["rot"][G:G + M].view(torch.int8), bufs["ph"][G:G + M].view(torch.int8)
        logits = bufs["q"][G:G + 4 * 7 * M].view(torch.float32).view(M, 7)
        rot, ph = pol.act(obs, ast, logits=logits)
        assert rot.data_ptr() == bufs["rot"].data_ptr() + G and ph.data_ptr() == bufs["ph"].data_ptr() + G
        rot, ph = rot.cpu().clone(), ph.cpu().clone()
        for k, b in bufs.items():
            assert bool((b[:G] == 0xFF).all()) and bool((b[-G:] == 0xFF).all()), k
        assert not bool(torch.isnan(logits).any())  # every q was written over the 0xFF fill (a NaN pattern)
        own = R.actions(logits.cpu(), 5)
        assert torch.equal(rot.long(), own[0]) and torch.equal(ph.long(), own[1])
        bufs["rot"].fill_(0xFF)
        bufs["ph"].fill_(0xFF)
        before = bufs["q"].clone()
        rot2, ph2 = pol.act(obs, ast, logits=None)  # no logits: the same actions, and the old buffer is left alone
        assert torch.equal(rot2.cpu(), rot) and torch.equal(ph2.cpu(), ph)
        assert torch.equal(bufs["q"], before)
        for k in ("rot", "ph"):
            assert bool((bufs[k][:G] == 0xFF).all()) and bool((bufs[k][-G:] == 0xFF).all()), k
    finally:
        pol._rot, pol._ph = keep


# ---- (g) reload ----------------------------------------------------------------------------------------------------------
def test_reload_collapses_again():
    import torch
    a, b = _fixture("init"), _fixture("spread")
    pol = _policy(a["sd"], 294)
    obs, ast = b["obs"][:64], b["ast"][:64]
    q_a, _, _ = _act(pol, obs, ast, "float32")
    pol.load_state_dict(b["sd"])
    q_b, rot_b, ph_b = _act(pol, obs, ast, "float32")
    fresh = _act(_policy(b["sd"], 294), obs, ast, "float32")
    assert same_bits(q_b, fresh[0]) and torch.equal(rot_b, fresh[1]) and torch.equal(ph_b, fresh[2])
    assert not same_bits(q_b, q_a)  # a stale collapsed buffer would still give the first model's q
    assert all(torch.equal(pol.state_dict()[k].cpu(), b["sd"][k]) for k in b["sd"])


# ---- (h) through the environment -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_through_the_environment(fmt):
    import torch
    f = _fixture("spread")
    pol = f["pol"]
    env = make_env(4, 64, dtype=getattr(torch, fmt))
    env.observe()
    q = torch.empty((256, 6), dtype=torch.float32, device="cuda")
    seen = set()
    for t in range(8):
        assert env.obs.shape == (4, 64, 7, 7, 6) and env.obs.dtype == getattr(torch, fmt)
        rot, ph = pol.act(env.obs, env.agent_state, logits=q, env=env)
        assert rot.shape == ph.shape == (4, 64)
        obs, ast = env.obs.float().cpu().reshape(256, 294), env.agent_state.cpu().reshape(256, 2)
        err, q64 = R.row_errors(f["sd"], obs, ast)
        _check_accuracy("env %s step %d" % (fmt, t), q.cpu(), q64, float(err.max()))
        own = R.actions(q.cpu(), 3)
        assert torch.equal(rot.cpu().reshape(-1).long(), own[0]) and torch.equal(ph.cpu().reshape(-1).long(), own[1])
        seen.add(obs.numpy().tobytes())
        env.step_update(rot, ph)  # the actions are accepted as they are
    assert len(seen) == 8  # the observations did move
