"""The rework population's entries alone, on synthetic inputs (antsrl_pop_rework_collapse, antsrl_pop_policy_rework,
antsrl_pop_policy_rework_select, antsrl_pop_reworktrain_step: antsrl_poprework.hip).  The contract is
identity with the single agent's entries on the member's own block, buffer, rows and slab, which the existing rework
tests hold to the reference: every comparison is torch.equal and no tolerance is involved.  The shapes are the smallest
at which each kernel can still go wrong; each is said where it is used."""
import ctypes as C

import numpy as np
import pytest

import memory_agent_ref as R
from agent_harness import ptr, stream
from population_harness import RING, population_trainer, synthetic_ring

pytestmark = pytest.mark.gpu

GUARD = 256  # canary bytes (or elements) on either side of an output
SMALL = dict(g1=8, g2=16, g3=8, r1=8, r2=16, r3=8, p1=8)


def _shape(F, n_rot=3, n_ph=3, **widths):
    """(AntsReworkShape, name -> (out, in) of the ten layers, trained floats NF, collapsed floats CF)."""
    from antsrl_amd import _lib
    from antsrl_amd.policy import rework_param_shapes
    layers = rework_param_shapes(F, n_rot, n_ph, **widths)
    a = dict(n_features=F, agent_dim=2, n_rot=n_rot, n_ph=n_ph, g1=layers["layer1"][0], g2=layers["layer2"][0], g3=layers["layer3"][0],
             r1=layers["rotation_layer1"][0], r2=layers["rotation_layer2"][0], r3=layers["rotation_layer3"][0],
             p1=layers["pheromone_layer1"][0])
    shp = _lib.AntsReworkShape(*[a[n] for n, _ in _lib.AntsReworkShape._fields_])
    return shp, layers, sum(o * i + o for o, i in layers.values()), (n_rot + n_ph) * (F + 3)


def _guarded(n, dtype, dev, fill):
    """(the whole buffer, its middle n elements): GUARD elements of `fill` on either side."""
    import torch
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _intact(whole, n, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def _check(rc, what):
    from antsrl_amd import _lib
    _lib.check(rc, what)


# ---- the collapse
@pytest.mark.parametrize("F,heads,widths", [(294, (3, 3), {}), (50, (5, 4), SMALL)], ids=["F294-3x3", "F50-5x4-small"])
def test_collapse_equals_the_single_collapse_per_member(F, heads, widths):
    """P = 3.  F = 294 with the reference's widths: CF = 1782 floats, so members 1 and 2 start 8 bytes off a 16-byte
    seam.  F = 50, heads (5, 4), small widths: NQ = 9 workgroups a member and every layer narrower than a workgroup."""
    import torch
    from antsrl_amd import _lib
    lib, dev, P = _lib.load(), torch.device("cuda", torch.cuda.current_device()), 3
    shp, layers, NF, CF = _shape(F, *heads, **widths)
    assert (F, CF) != (294, 1782) or CF % 4 == 2
    g = torch.Generator(device="cpu")
    g.manual_seed(F)
    blocks = ((torch.rand((P, NF), generator=g) * 2 - 1) * 0.2).to(dev)
    whole, out = _guarded(P * CF, torch.float32, dev, -7.0)
    _check(lib.antsrl_pop_rework_collapse(C.byref(shp), P, ptr(blocks), ptr(out), stream()), "pop_rework_collapse")
    for p in range(P):
        ptrs, off = [], 0
        for o, i in layers.values():
            ptrs += [blocks[p].data_ptr() + 4 * off, blocks[p].data_ptr() + 4 * (off + o * i)]
            off += o * i + o
        assert off == NF
        alone = torch.full((CF,), -3.0, dtype=torch.float32, device=dev)
        _check(lib.antsrl_rework_collapse(C.byref(shp), (C.c_void_p * 20)(*ptrs), ptr(alone), stream()), "rework_collapse")
        assert torch.equal(out[p * CF:(p + 1) * CF], alone), ("collapsed", p)
    assert _intact(whole, P * CF, -7.0), "the guards around the [P] buffer"
    assert len({out[p * CF:(p + 1) * CF].cpu().numpy().tobytes() for p in range(P)}) == P


# ---- acting
#: P, Em, N, F, heads, epsilons, seeds.  (a): Mm = 40: the pass of 8 rows at rows 16-23 straddles two colonies; member 2's
#: passes all explore, member 0's never.  (b): Mm = 20: the last pass has 4 valid rows.  (c): heads (5, 4): the NQP = 16
#: instantiation.  (d): F = 50 < 64: no full chunk, everything goes through the tail loads.
ACT = dict(a=(3, 2, 20, 294, (3, 3), (0.0, 0.5, 1.0), (7, 8, 7)), b=(2, 2, 10, 294, (3, 3), (0.5, 0.5), (7, 9)),
           c=(2, 1, 32, 294, (5, 4), (0.5, 0.5), (7, 9)), d=(2, 1, 8, 50, (3, 3), (0.5, 0.5), (7, 9)))


def _mixed_step(seed, env_base, Em, eps):
    """The first step at which a member's colonies do not all get the same explore flag (antsrl_draw.h restated in
    memory_agent_ref), or step 3 for a member of one colony."""
    for step in range(64):
        ex = R.explores(seed, step, env_base, Em, eps)
        if Em > 1 and ex.any() and not ex.all():
            return step
    assert Em == 1
    return 3


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", sorted(ACT))
def test_acting_equals_the_single_entries_per_member(case, bf16):
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.population import _Geometry
    lib, dev = _lib.load(), torch.device("cuda", torch.cuda.current_device())
    P, Em, N, F, heads, eps, seeds = ACT[case]
    Mm, M, NQ, fmt = Em * N, P * Em * N, sum(heads), 1 if bf16 else 0
    assert (Mm * F * (2 if bf16 else 4)) % 16 == 0  # the entry's slice rule
    shp, _, _, CF = _shape(F, *heads)
    g = torch.Generator(device="cpu")
    g.manual_seed(17 * F + M)
    collapsed = ((torch.rand((P, CF), generator=g) * 2 - 1) * 0.1).to(dev)
    obs = (torch.rand((M, F), generator=g) * 2 - 1).to(dev, torch.bfloat16 if bf16 else torch.float32)
    ast = torch.rand((M, 2), generator=g).to(dev)
    spec = _Geometry(P, P * Em, N, 0, F, obs.dtype).spec(seeds, eps, [1e-3] * P, [0.5] * P)
    step = _mixed_step(seeds[1], Em, Em, eps[1])
    want_ex = np.concatenate([R.explores(seeds[p], step, p * Em, Em, eps[p]) for p in range(P)])
    if case == "a":
        assert list(want_ex[:2]) == [False, False] and want_ex[2] != want_ex[3] and list(want_ex[4:]) == [True, True]

    def alone(p, sel):
        """The single entries on member p's slice with its own collapsed buffer."""
        rows = slice(p * Mm, (p + 1) * Mm)
        o, a = obs[rows].contiguous(), ast[rows].contiguous()
        rot, ph = (torch.full((Mm,), 99, dtype=torch.int8, device=dev) for _ in range(2))
        q = torch.full((Mm, NQ), -5.0, dtype=torch.float32, device=dev)
        ex = torch.full((Em,), 9, dtype=torch.uint8, device=dev)
        if sel:
            _check(lib.antsrl_policy_rework_select(C.byref(shp), ptr(collapsed[p]), ptr(o), fmt, ptr(a), seeds[p], step, p * Em, Em, N,
                                                   float(eps[p]), ptr(rot), ptr(ph), ptr(ex), ptr(q), stream()), "policy_rework_select")
        else:
            _check(lib.antsrl_policy_rework(C.byref(shp), ptr(collapsed[p]), ptr(o), fmt, ptr(a), Mm, ptr(rot), ptr(ph), ptr(q),
                                            stream()), "policy_rework")
        return rot, ph, q, ex

    for sel in (False, True):
        w_rot, rot = _guarded(M, torch.int8, dev, 99)
        w_ph, ph = _guarded(M, torch.int8, dev, 99)
        w_ex, ex = _guarded(P * Em, torch.uint8, dev, 9)
        w_q, q = _guarded(M * NQ, torch.float32, dev, -5.0)
        if sel:
            _check(lib.antsrl_pop_policy_rework_select(C.byref(spec), C.byref(shp), ptr(collapsed), ptr(obs), ptr(ast), step, ptr(rot),
                                                       ptr(ph), ptr(ex), ptr(q), stream()), "pop_policy_rework_select")
            assert torch.equal(ex.cpu(), torch.from_numpy(want_ex.astype(np.uint8))), "the flags are the draw specification's"
        else:
            _check(lib.antsrl_pop_policy_rework(C.byref(spec), C.byref(shp), ptr(collapsed), ptr(obs), ptr(ast), ptr(rot), ptr(ph),
                                                ptr(q), stream()), "pop_policy_rework")
        for p in range(P):
            rows = slice(p * Mm, (p + 1) * Mm)
            a_rot, a_ph, a_q, a_ex = alone(p, sel)
            # a clamp or a last_dword that crosses a member shows in its first and last rows
            for name, r in (("first", p * Mm), ("last", (p + 1) * Mm - 1)):
                assert int(rot[r]) == int(a_rot[r - p * Mm]) and int(ph[r]) == int(a_ph[r - p * Mm]), (name, "row of member", p, sel)
                assert torch.equal(q[r * NQ:(r + 1) * NQ], a_q[r - p * Mm]), (name, "row's q of member", p, sel)
            assert torch.equal(rot[rows], a_rot) and torch.equal(ph[rows], a_ph), ("actions", p, sel)
            assert torch.equal(q[p * Mm * NQ:(p + 1) * Mm * NQ].view(Mm, NQ), a_q), ("q", p, sel)
            if sel:
                assert torch.equal(ex[p * Em:(p + 1) * Em], a_ex), ("explored", p)
        if sel and eps[0] == 0.0:  # a member that never explores gets k_rework_act's bits from the select entry
            plain = alone(0, False)
            assert torch.equal(rot[:Mm], plain[0]) and torch.equal(ph[:Mm], plain[1]) and torch.equal(q[:Mm * NQ].view(Mm, NQ), plain[2])
        assert _intact(w_rot, M, 99) and _intact(w_ph, M, 99) and _intact(w_q, M * NQ, -5.0), ("guards", sel)
        assert _intact(w_ex, P * Em, 9) and (sel or bool((ex == 9).all())), ("explored", sel)


# ---- the training step
def _train_case(B, P, dev):
    """Two consecutive steps of a PopulationReworkTrainer (distinct discounts and learning rates, a target that is not the
    model) on a float32 ring of 256 rows a member, and what they left."""
    import torch
    F, L = 294, 256
    seeds, discount, lr = (7, 8, 7)[:P], (0.5, 0.99, 0.9)[:P], (1e-3, 1e-4, 3e-3)[:P]
    ring = synthetic_ring(3, L, (F,), dev, seed=11)
    g = torch.Generator(device="cpu")
    g.manual_seed(B)
    idx = [torch.randint(0, L, (3, B), generator=g).to(dev) for _ in range(2)]
    target0 = None
    tr = population_trainer("PopulationReworkTrainer", P, (F,), dev, seeds, discount, lr)
    g.manual_seed(5)
    target0 = ((torch.rand((3, tr.trained_floats), generator=g) * 2 - 1) * 0.1).to(dev)
    tr.target.copy_(target0[:P])
    tr._collapse()
    sub = ring if P == 3 else _first_member(ring, dev)
    keep = dict(target=tr.target.clone(), collapsed=tr.collapsed.clone(), version=tr.version)
    init = [tr.state_dict(p) for p in range(P)]
    tf, stride, ws, launches, cf = tr._sizes(B)
    assert launches == 4 and ws == P * stride and stride % 256 == 0
    losses = [tr.step(sub, idx[0][:P].contiguous()).clone()]
    first = dict(model=tr.model.clone(), grads=tr.grads.clone(), adam=tr._adam.clone(), rl=tr.running_loss.clone(), work=tr._work.clone())
    losses.append(tr.step(sub, idx[1][:P].contiguous()).clone())
    torch.cuda.synchronize()
    return dict(tr=tr, ring=ring, idx=idx, target0=target0, keep=keep, init=init, stride=stride, cf=cf, losses=losses, first=first,
                seeds=seeds, discount=discount, lr=lr)


def _first_member(ring, dev):
    """Member 0's slab as a population ring of one member."""
    from antsrl_amd.population import PopulationReplayMemory
    one = PopulationReplayMemory(1, ring.max_len, ring.observation_space, device=dev)
    for n in RING:
        getattr(one, n).copy_(getattr(ring, n)[:1])
    one.fill = ring.fill
    return one


#: B = 40: three passes, the last with 8 valid rows.  48: three whole passes.  264: the reference's.  4112: 257 passes on
#: 256 parts, so workgroup 0 loops.
@pytest.mark.parametrize("B", [40, 48, 264, 4112])
def test_the_step_equals_a_lone_trainer_s_per_member(B):
    import torch
    from antsrl_amd.train import ReworkTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    F, P = 294, 3
    c = _train_case(B, P, dev)
    tr, ring, idx, losses, first, stride, cf = c["tr"], c["ring"], c["idx"], c["losses"], c["first"], c["stride"], c["cf"]
    assert bool(torch.isfinite(torch.stack(losses)).all()) and not torch.equal(first["model"], tr.model)
    assert torch.equal(tr.target, c["keep"]["target"]) and torch.equal(tr.collapsed, c["keep"]["collapsed"]), \
        "a step leaves the target and its collapsed buffer"
    assert tr.version == c["keep"]["version"] and tr.step_count == 2
    assert torch.equal(first["rl"], losses[0].double()), "the first training step's running loss is its loss"
    # the second step (first = 0): main.py:106-109 in float64, each product rounded before the add
    assert torch.equal(tr.running_loss, 0.99 * first["rl"] + 0.01 * losses[1].double())
    assert not torch.equal(tr.running_loss, first["rl"])
    for p in range(P):
        one = ReworkTrainer(F, dev, discount=c["discount"][p], lr=c["lr"][p], update_target_every=1000, seed=c["seeds"][p])
        sd0 = one.state_dict()
        assert list(sd0) == list(c["init"][p]) and all(torch.equal(sd0[k], c["init"][p][k]) for k in sd0), \
            "member %d is initialised as ReworkPolicy(seed)" % p
        one.target.copy_(c["target0"][p])
        one.policy.recollapse()
        assert torch.equal(one.policy.collapsed, c["keep"]["collapsed"][p]), ("the target's collapsed buffer", p)
        slab = tuple(getattr(ring, n)[p] for n in RING)
        l0 = one.step(slab, idx[0][p])
        assert torch.equal(l0, losses[0][p]), ("loss", p, 0, float(l0), float(losses[0][p]))
        for name, mine, alone in (("model", first["model"][p], one.model), ("grads", first["grads"][p], one.grads),
                                  ("adam m", first["adam"][0, p], one._adam[0]), ("adam v", first["adam"][1, p], one._adam[1])):
            assert torch.equal(mine, alone), (name, p, "after the first step")
        # the workspace's collapsed buffer (the MODEL's, as the down chain found it) leads a member's part
        mine = first["work"][p * stride: p * stride + 4 * cf].view(torch.float32)
        assert torch.equal(mine, one._work[:4 * cf].view(torch.float32)), ("the workspace's collapsed buffer", p, 0)
        l1 = one.step(slab, idx[1][p])
        assert torch.equal(l1, losses[1][p]), ("loss", p, 1, float(l1), float(losses[1][p]))
        for name, mine, alone in (("model", tr.model[p], one.model), ("grads", tr.grads[p], one.grads),
                                  ("adam m", tr._adam[0, p], one._adam[0]), ("adam v", tr._adam[1, p], one._adam[1]),
                                  ("target", tr.target[p], one.target)):
            assert torch.equal(mine, alone), (name, p, "after the second step")
        mine = tr._work[p * stride: p * stride + 4 * cf].view(torch.float32)
        assert torch.equal(mine, one._work[:4 * cf].view(torch.float32)), ("the workspace's collapsed buffer", p, 1)
        ad, alone_ad = tr.adam_state(p), one.adam_state()
        assert ad["step"] == alone_ad["step"] == 2
        assert all(torch.equal(ad[m][k], alone_ad[m][k]) for m in ("exp_avg", "exp_avg_sq") for k in ad[m])
        sd, alone_sd = tr.state_dict(p), one.state_dict()
        assert list(sd) == list(alone_sd) and len(sd) == 20 and all(torch.equal(sd[k], alone_sd[k]) for k in sd)
    if B == 40:  # a member inside P = 3 and inside P = 1: equal bits
        c1 = _train_case(B, 1, dev)
        t1 = c1["tr"]
        for name, a, b in (("model", t1.model[0], tr.model[0]), ("grads", t1.grads[0], tr.grads[0]), ("adam", t1._adam[:, 0], tr._adam[:, 0]),
                           ("running loss", t1.running_loss[0], tr.running_loss[0]), ("loss 0", c1["losses"][0][0], losses[0][0]),
                           ("loss 1", c1["losses"][1][0], losses[1][0])):
            assert torch.equal(a, b), (name, "of member 0 inside P = 1 and P = 3")
