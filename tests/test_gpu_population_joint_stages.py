"""The joint population's training step alone (antsrl_pop_jointtrain_step: k_pop_jointtrain_fwd and k_pop_jointtrain_l1,
antsrl_popjoint.hip), off the fused loop's two shapes, on population_harness.synthetic_ring with per-member
discounts and learning rates that differ.

Every member is held twice: bit for bit to a lone JointTrainer stepped on the same rows — model, Adam's moments, grads,
loss, running loss and the member's whole part of the workspace (partials and dh) — and to the float64 restatement under
the bounds that are already in the tree, joint_train_ref.fp32_sum_bounds and partial_bounds (derived, not measured:
test_joint_train_bounds_cpu.py shows them safe and sharp).  The workspace is pattern-filled: what no stage writes keeps the
pattern, and a zero-filled and an 0xff-filled workspace give equal bits."""
import pytest

import joint_train_ref as J
import population_stage_cases as S
from population_harness import RING, population_trainer, synthetic_ring
from test_gpu_population_joint import JOINT as H

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
LDS_PLAIN = 64 * 1024


def jt_lds(F):
    """antsrl_jointtrain_dev.h's jt_lds at ksteps = ceil(F / 16): the bf16 image of W1 [32][16 ksteps + 8], the three head
    slots (304 floats), b1 and two columns of W1 (96), four waves' partial sums (4 x 200) and four tiles of h [32][33]
    and dq [32][8]."""
    ks = (F + 15) // 16
    return 32 * (16 * ks + 8) * 2 + (304 + 96 + 4 * 200 + 4 * (32 * 33 + 32 * 8)) * 4


FIRST_OPT_IN = next(F for F in range(1, 1023) if jt_lds(F) > LDS_PLAIN)

#: (F, B, P).  (9, 1, 3): one row.  (17, 33, 3): a second tile with one row.  (294, 136, 2): two forward workgroups.
#: (294, 512, 64): four forward workgroups and P at its maximum.  (609, 33, 2): the first F whose LDS exceeds 64 KiB.
#: (848, 40, 2): the widest acting row.
CASES = [(9, 1, 3), (17, 33, 3), (294, 136, 2), (294, 512, 64), (FIRST_OPT_IN, 33, 2), (848, 40, 2)]


def test_the_cases_are_what_they_are_for():
    assert FIRST_OPT_IN == 609 and jt_lds(608) <= LDS_PLAIN < jt_lds(609)
    for F in sorted({c[0] for c in CASES} | {608, 1022}):
        assert jt_lds(F) == J.lds_bytes(F), F
    assert [J.blocks(B) for _, B, _ in CASES] == [1, 1, 2, 4, 1, 1]
    assert S.pol_flat_fits(848) and not S.pol_flat_fits(849) and max(P for _, _, P in CASES) == S.POP_MAX


def _cycle(values, P):
    return tuple(values[p % len(values)] for p in range(P))


def _share(err, bound):
    import torch
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


def _bits(t):
    import torch
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


@pytest.mark.parametrize("F,B,P", CASES, ids=["F%d-B%d-P%d" % c for c in CASES])
def test_the_step_alone(F, B, P):
    import torch
    from antsrl_amd.train import JointTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    L = 600
    seeds, discount, lr = _cycle(S.TRAIN_SEEDS, P), _cycle(S.TRAIN_DISCOUNT, P), _cycle(S.TRAIN_LR, P)
    assert len(set(discount[:2])) == 2 and len(set(lr[:2])) == 2
    ring = synthetic_ring(P, L, (F,), dev, seed=11)
    g = torch.Generator(device="cpu")
    g.manual_seed(1000 * F + B)
    idx = [torch.randint(0, L, (P, B), generator=g).to(dev) for _ in range(2)]
    target0 = ((torch.rand((P, 99), generator=g) * 2 - 1) * 0.3).to(dev)  # a target layer3 that is not the live one
    W = J.work_layout(B)
    nb, dh_off, used = W["blocks"], W["dh_offset"], W["bytes"]

    def run(fill):
        """Two consecutive steps on a workspace filled with `fill`, with a guard behind it."""
        tr = population_trainer("PopulationJointTrainer", P, (F,), dev, seeds, discount, lr)
        tf, stride, ws, launches = tr._sizes(B)
        assert tf == 32 * (F + 2) + 230 and launches == 2 and ws == P * stride and stride % 256 == 0 and used <= stride < used + 256
        tr.target_l3.copy_(target0)
        init = [tr.state_dict(p) for p in range(P)]
        big = torch.full((ws + 1024,), fill, dtype=torch.uint8, device=dev)
        tr._work, tr._work_B = big[:ws], B
        assert big.data_ptr() % 256 == 0
        losses = [tr.step(ring, idx[0]).clone()]
        first = dict(model=tr.model.clone(), grads=tr.grads.clone(), adam=tr._adam.clone(), rl=tr.running_loss.clone(),
                     work=big.clone())
        losses.append(tr.step(ring, idx[1]).clone())
        torch.cuda.synchronize()
        return tr, big, stride, losses, first, init

    tr, big, stride, losses, first, init = run(PATTERN)
    assert bool(torch.isfinite(torch.stack(losses)).all()) and not torch.equal(first["model"], tr.model)
    assert torch.equal(tr.target_l3, target0), "a step leaves the target's layer3"
    assert torch.equal(first["rl"], losses[0].double()), "the first training step's running loss is its loss"
    # the second step (first = 0): main.py:106-109 in float64, each product rounded before the add
    assert torch.equal(tr.running_loss, 0.99 * first["rl"] + 0.01 * losses[1].double())
    assert not torch.equal(tr.running_loss, first["rl"])

    def parts(work, p=0):
        """Member p's partials [blocks, 199] and dh [B, 32] (float32) in a population's workspace, or a lone step's."""
        part = work[p * stride: p * stride + used]
        return (part[: nb * J.PART * 4].view(torch.float32).view(nb, J.PART)[:, :J.OUT],
                part[dh_off: used].view(torch.float32).view(B, 32))

    worst = dict(g=0.0, l=0.0, dh=0.0, part=0.0)
    for p in range(P):
        # ---- a lone JointTrainer on the member's slab
        one = JointTrainer(F, dev, discount=discount[p], lr=lr[p], update_target_every=1000, seed=seeds[p])
        one.target_l3.copy_(target0[p])
        sd0 = one.state_dict()
        assert all(torch.equal(sd0[k], init[p][k]) for k in sd0), ("member %d is initialised as JointTrainer(seed)" % p)
        slab = tuple(getattr(ring, n)[p] for n in RING)
        l0 = one.step(slab, idx[0][p])
        assert torch.equal(l0, losses[0][p]), ("loss", p, 0, float(l0), float(losses[0][p]))
        for name, mine, alone in (("model", first["model"][p], one.model), ("grads", first["grads"][p], one.grads),
                                  ("adam m", first["adam"][0, p], one._adam[0]), ("adam v", first["adam"][1, p], one._adam[1])):
            assert torch.equal(mine, alone), (name, p, "after the first step")
        part, dh = parts(first["work"], p)
        one_part, one_dh = parts(one._work)
        assert torch.equal(_bits(part), _bits(one_part)), ("partials", p)
        assert torch.equal(_bits(dh), _bits(one_dh)), ("dh", p)
        # what neither stage writes kept the pattern: float 199 of every row of partials, the gap in front of dh, and
        # the bytes between the member's used part and the next stride
        mine = first["work"][p * stride:(p + 1) * stride]
        rows = mine[: nb * J.PART * 4].view(nb, J.PART * 4)
        assert bool((rows[:, J.OUT * 4:] == PATTERN).all()), ("the partials' pad", p)
        assert bool((mine[nb * J.PART * 4: dh_off] == PATTERN).all()), ("the gap in front of dh", p)
        assert bool((mine[used:] == PATTERN).all()), ("the stride's tail", p)
        # ---- the first step against float64, under the tree's derived bounds
        sd = {k: v.cpu() for k, v in init[p].items()}
        state = J.new_state(sd, (target0[p, :96].view(3, 32).cpu(), target0[p, 96:].cpu()))
        rows_p = idx[0][p].cpu()
        batch = tuple(a.cpu()[rows_p] for a in slab)
        loss_ref, g_ref = J.contract_train_step(state, batch, discount[p], update=False)
        bound = J.fp32_sum_bounds(state, batch, discount[p])
        gd = {k: v.cpu() for k, v in tr._views(first["grads"][p]).items()}
        share = J.worst_share(gd, g_ref, bound)
        loss = float(losses[0][p])
        share_l = abs(loss - loss_ref) / bound["loss"] if loss != loss_ref else 0.0
        _, dh_ref = J.contract_backward(state, J.contract_forward(state, batch, discount[p]))
        share_dh = _share((dh.cpu().double() - dh_ref.double()).abs(), bound["dh"])
        share_p = _share((part.cpu().double() - J.expected_partials(state, batch, discount[p])).abs(),
                         J.partial_bounds(state, batch, discount[p]))
        for key, v in (("g", share), ("l", share_l), ("dh", share_dh), ("part", share_p)):
            worst[key] = max(worst[key], v)
        if p == P - 1:
            print("\nMEASURED F %d B %d P %d: worst share over the members of the fp32 sum bound: gradient %.3g, loss %.3g, dh %.3g; "
                  "partials %.3g of their own" % (F, B, P, worst["g"], worst["l"], worst["dh"], worst["part"]))
        assert share <= 1.0 and share_l <= 1.0 and share_dh <= 1.0 and share_p <= 1.0, (p, share, share_l, share_dh, share_p)
        # ---- the second step, on the weights and moments the first one moved
        l1 = one.step(slab, idx[1][p])
        assert torch.equal(l1, losses[1][p]), ("loss", p, 1, float(l1), float(losses[1][p]))
        H.same_trainers(tr, p, one)
        assert tr.step_count == one.step_count == 2
        part2, dh2 = parts(big, p)
        one_part2, one_dh2 = parts(one._work)
        assert torch.equal(_bits(part2), _bits(one_part2)) and torch.equal(_bits(dh2), _bits(one_dh2)), ("the workspace after step 2", p)
    assert bool((big[P * stride:] == PATTERN).all()), "the guard behind the workspace"

    # a zero-filled and an 0xff-filled workspace give equal bits (and the pattern-filled one's)
    outs = []
    for fill in (0x00, 0xFF):
        tr2, big2, stride2, losses2, first2, _ = run(fill)
        assert stride2 == stride and bool((big2[P * stride:] == fill).all())
        for p in range(P):
            for a, b in zip(parts(first2["work"], p) + parts(big2, p), parts(first["work"], p) + parts(big, p)):
                assert torch.equal(_bits(a), _bits(b)), ("the workspace under fill %#x" % fill, p)
        outs.append((tr2.model, tr2.grads, tr2._adam, tr2.running_loss, first2["model"], first2["grads"], first2["adam"],
                     losses2[0], losses2[1]))
    ref = (tr.model, tr.grads, tr._adam, tr.running_loss, first["model"], first["grads"], first["adam"], losses[0], losses[1])
    for out in outs:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, ref))
