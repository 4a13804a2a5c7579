"""The joint training step on the device: JointTrainer (antsrl_jointtrain_step: layer1 trained under the
collect heads) against the device-contract restatement, stage by stage from its workspace, against the reference's
arithmetic and against the reference's own recording (tests/joint_train_ref.py, tests/golden/contract/joint_train_ref.npz).
Every bound is joint_train_ref's, from the restatement and the inputs alone; -s prints the worst share of each per case."""
import math
import os

import numpy as np
import pytest

import dqn_ref as D
import explore_train_ref as X
import joint_train_ref as J
from agent_harness import param_tolerance as _param_tolerance
from agent_harness import same_bits as _same_bits

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "joint_train_ref.npz")


def _trainer(state, F, discount=0.5, lr=1e-4):
    """A JointTrainer holding state's model and its (different) target layer3."""
    from antsrl_amd.train import JointTrainer
    tr = JointTrainer(F, "cuda", discount=discount, lr=lr)
    tr.load_state_dict(state["sd"])
    tr.target_l3[0:96].copy_(state["target_w3"].reshape(-1))
    tr.target_l3[96:99].copy_(state["target_b3"])
    return tr


def _cases():
    for F, B in J.SHAPES:
        yield "F%d_B%d" % (F, B)
    for name in J.VARIANTS:
        yield name


def _make(name):
    """(state, device arrays, device idx or None, discount, B, F, the gathered batch of the restatement)."""
    if name in J.VARIANTS:
        state, arrays, idx, discount, B = J.make_variant(name)
        F = 17
    else:
        F, B = (int(s[1:]) for s in name.split("_"))
        state, arrays, idx = J.shape_case(F, B)
        discount = 0.5
    batch = J.gather_clamped(arrays, idx, B)
    dev = tuple(a.cuda().contiguous() for a in arrays)
    return state, dev, (None if idx is None else idx.cuda()), discount, B, F, batch


def _workspace(tr, B):
    """(partials [workgroups][199], dh [B][32]) read back from the trainer's workspace, on the CPU."""
    import torch
    W = J.work_layout(B)
    work = tr._work.cpu()
    part = work[: W["blocks"] * J.PART * 4].view(torch.float32).view(W["blocks"], J.PART)[:, :J.OUT].clone()
    return part, work[W["dh_offset"]: W["bytes"]].view(torch.float32).view(B, 32).clone()


def _share(err, bound):
    import torch
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ---- 1. the step against the contract, stage by stage, and equal inputs give equal bits
@pytest.mark.parametrize("name", list(_cases()))
def test_step_equals_the_contract_stage_by_stage(name):
    import torch
    state, dev, idx, discount, B, F, batch = _make(name)
    loss_ref, g_ref = J.contract_train_step(state, batch, discount, update=False)
    bound = J.fp32_sum_bounds(state, batch, discount)  # from the restatement and the inputs alone
    tr = _trainer(state, F, discount)
    assert tr.launches(B) == 2 and tr.trained_floats == 32 * (F + 2) + 230
    target0 = tr.target_l3.clone()
    tr.grads.fill_(SENTINEL)
    before = {k: v.cpu() for k, v in tr.state_dict().items()}
    v0 = tr.version
    loss_t = tr.step(dev, idx)
    loss = float(loss_t)
    assert tr.version == v0 + 1
    gd = {k: v.cpu() for k, v in tr.grad_dict().items()}
    share = J.worst_share(gd, g_ref, bound)
    share_l = abs(loss - loss_ref) / bound["loss"] if loss != loss_ref else 0.0
    # dh, read back, against the contract's, inside its own bound
    part, dh = _workspace(tr, B)
    f = J.contract_forward(state, batch, discount)
    _, dh_ref = J.contract_backward(state, f)
    share_dh = _share((dh.double() - dh_ref.double()).abs(), bound["dh"])
    # layer1's gradient against float64 dh^T xe on the device's OWN dh: what is left is the layer1 stage's summation,
    # ceil(B / 16) fmafs and 15 adds per element and this comparison's rounding: gamma(ceil(B / 16) + 16) sum |dh| |xe|
    xe1 = torch.cat([f["xe"], torch.ones((B, 1))], 1).double()
    want = dh.double().T @ xe1
    lim = D.gamma(math.ceil(B / 16) + 16) * (dh.double().abs().T @ xe1.abs())
    got = torch.cat([gd[J.W1], gd[J.B1][:, None]], 1).double()
    share_l1 = _share((got - want).abs(), lim)
    # every workgroup's row of partials against the contract's, inside the per-partial bound
    share_p = _share((part.double() - J.expected_partials(state, batch, discount)).abs(), J.partial_bounds(state, batch, discount))
    # the 198 head gradients and the loss: the ordered fp32 sum of the device's own partials, bit for bit
    total = J.ordered_sum(part)
    heads = torch.cat([gd[k].reshape(-1) for k in J.NAMES[2:]])
    assert _same_bits(total[:198], heads) and _same_bits(total[198:199], loss_t.cpu().reshape(1))
    # Adam from the device's own gradient: the moments bit for bit (the first step from a zero Adam state)
    J.adam(state, gd, tr.lr, tr.betas, tr.eps)
    st, after = tr.adam_state(), tr.state_dict()
    worst_p = 0.0
    for k in J.NAMES:
        assert torch.equal(st["exp_avg"][k].cpu(), state["m"][k]) and torch.equal(st["exp_avg_sq"][k].cpu(), state["v"][k]), k
        err = (after[k].cpu() - state["sd"][k]).abs()
        worst_p = max(worst_p, float((err / _param_tolerance(state["sd"][k], before[k])).max()))
    print("\nMEASURED %-16s share of the fp32 sum bound: gradient %.3g, loss %.3g, dh %.3g; partials %.3g and layer1 stage %.3g "
          "of their own; parameters %.3g of their tolerance" % (name, share, share_l, share_dh, share_p, share_l1, worst_p))
    assert np.isfinite(loss) and share <= 1.0 and share_l <= 1.0 and share_dh <= 1.0 and share_l1 <= 1.0 and worst_p <= 1.0
    assert share_p <= 1.0
    assert not bool((tr.grads == SENTINEL).any())
    assert torch.equal(tr.target_l3, target0)  # the target's layer3 is only read
    # the same step on a fresh trainer: equal bits
    state0 = _make(name)[0]
    tw = _trainer(state0, F, discount)
    loss_w = tw.step(dev, idx)
    assert _same_bits(loss_w.reshape(1), loss_t.reshape(1))
    assert torch.equal(tw.model, tr.model) and torch.equal(tw._adam, tr._adam) and torch.equal(tw.grads, tr.grads)
    part_w, dh_w = _workspace(tw, B)
    assert _same_bits(part_w, part) and _same_bits(dh_w, dh)


# ---- 2. grad() + apply(), step() and step(keep_grads=False)
@pytest.mark.parametrize("F,B", [(294, 264), (17, 513)])
def test_grad_apply_step_and_step_without_grads_give_equal_bits(F, B):
    import torch
    state, arrays, idx = J.shape_case(F, B)
    dev, idx = tuple(a.cuda().contiguous() for a in arrays), idx.cuda()
    runs = {}
    for mode in ("step", "grad_apply", "no_grads"):
        tr = _trainer(J.shape_case(F, B)[0], F)
        tr.grads.fill_(SENTINEL)
        losses = []
        for _ in range(2):  # the second step starts from a non-zero Adam state
            if mode == "grad_apply":
                losses.append(float(tr.grad(dev, idx)))
                tr.apply()
            else:
                losses.append(float(tr.step(dev, idx, keep_grads=mode != "no_grads")))
        runs[mode] = (losses, tr)
    l0, t0 = runs["step"]
    assert l0[0] != l0[1] and t0.step_count == 2
    for mode in ("grad_apply", "no_grads"):
        losses, tr = runs[mode]
        assert losses == l0, mode
        assert torch.equal(tr.model, t0.model) and torch.equal(tr._adam, t0._adam) and torch.equal(tr.target_l3, t0.target_l3), mode
        if mode == "no_grads":
            assert bool((tr.grads == SENTINEL).all())
        else:
            assert torch.equal(tr.grads, t0.grads), mode


# ---- 3. the workspace: nothing is read before it is written, nothing is written outside the layout
@pytest.mark.parametrize("F,B", [(17, 33), (294, 513)])
def test_workspace_of_zero_bytes_and_of_ff_bytes_between_guards(F, B):
    import torch
    state, arrays, idx = J.shape_case(F, B)
    dev, idx = tuple(a.cuda().contiguous() for a in arrays), idx.cuda()
    W, G = J.work_layout(B), 4096
    got = []
    for fill in (0x00, 0xFF):
        tr = _trainer(J.shape_case(F, B)[0], F)
        buf = torch.full((G + W["bytes"] + G,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 256 == 0
        buf[G: G + W["bytes"]] = fill
        tr._work = buf[G: G + W["bytes"]]  # exactly workspace_bytes: the guard starts behind dh's row B - 1
        loss = tr.step(dev, idx)
        assert tr._work.data_ptr() == buf.data_ptr() + G
        assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + W["bytes"]:] == 0xA5).all())
        got.append((loss.clone(), tr.model.clone(), tr._adam.clone(), tr.grads.clone()))
    for a, b in zip(*got):
        assert _same_bits(a.reshape(-1), b.reshape(-1))


# ---- 4. the twin: with layer3 all zero the step is the explore agent's on layer1 and layer2
@pytest.mark.parametrize("F,B", [(294, 264), (17, 513)])
def test_twin_with_a_zero_layer3_equals_the_explore_trainer(F, B):
    """layer3 and its target all zero: q_ph = y_ph's net part = 0, dq_ph * w3[a_ph][j] = +-0 and dh = dq_rot * w2[a_rot][j]
    +- 0; an ExploreTrainer whose target equals its model computes h' through the same layer1 and takes the same layer2's
    maximum.  Stage 2 is the same device code.  So g_w1, g_b1 and layer2's gradients compare equal."""
    import torch
    from antsrl_amd.train import ExploreTrainer
    state, arrays, idx = J.shape_case(F, B)
    sd = state["sd"]
    sd[J.W3].zero_()
    sd[J.B3].zero_()
    state["target_w3"].zero_()
    state["target_b3"].zero_()
    dev, idx = tuple(a.cuda().contiguous() for a in arrays), idx.cuda()
    tj = _trainer(state, F)
    te = ExploreTrainer(F, "cuda")
    te.load_state_dict({k: sd["explore_model." + k] for k in X.NAMES})  # model and target
    tj.step(dev, idx)
    te.step(dev, idx)
    gj, ge = tj.grad_dict(), te.grad_dict()
    for k in X.NAMES:
        assert bool((gj["explore_model." + k] == ge[k]).all()), k
        assert float(ge[k].abs().max()) > 0
    _, dh_j = _workspace(tj, B)
    W = X.work_layout(B)
    dh_e = te._work.cpu()[W["dh_offset"]: W["bytes"]].view(torch.float32).view(B, 32)
    assert bool((dh_j == dh_e).all())


# ---- 5. against the reference's arithmetic, in fp32
def test_twenty_steps_against_the_references_arithmetic():
    import torch
    F, B = 294, 264
    state, arrays, _ = J.make_case(F, B, 77, N=2000)
    dev = tuple(a.cuda().contiguous() for a in arrays)
    tr = _trainer(state, F)
    g = torch.Generator().manual_seed(5)
    worst = worst_l = 0.0
    for s in range(20):
        idx = torch.randint(0, 2000, (B,), generator=g)
        batch = J.gather(arrays, idx)
        # each step is compared from the device's own weights: the bound is that of ONE step's bfloat16 roundings
        tsd = tr.target_state_dict()
        host = J.new_state({k: v.cpu() for k, v in tr.state_dict().items()}, (tsd[J.W3].cpu(), tsd[J.B3].cpu()))
        bd = J.bf16_bounds(host, batch)
        loss_ref, g_ref = J.fp32_train_step(host, batch, update=False)
        loss = float(tr.train_on(dev, idx.cuda(), done=(s % 7 == 6)))
        worst = max(worst, J.worst_share({k: v.cpu() for k, v in tr.grad_dict().items()}, g_ref, bd))
        worst_l = max(worst_l, abs(loss - loss_ref) / bd["loss"])
    print("\nMEASURED 20 steps at (294, 264) against torch fp32 autograd: worst share of the bf16 bound, gradient %.3g, loss %.3g"
          % (worst, worst_l))
    assert worst <= 1.0 and worst_l <= 1.0 and tr.syncs == 2 and tr.step_count == 20


# ---- 6. against the reference's own recording
def test_the_three_recorded_calls():
    import torch
    fx = np.load(FIXTURE)
    F = 294
    names = ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")
    dev = tuple(torch.as_tensor(fx["rows/" + k]).cuda().contiguous() for k in names)
    dev = (dev[0].reshape(len(dev[3]), -1), *dev[1:4], dev[4].reshape(len(dev[3]), -1), *dev[5:])
    from antsrl_amd.train import JointTrainer
    tr = JointTrainer(F, "cuda", state_dict={k: fx["init/" + k] for k in J.NAMES})
    host = J.new_state({k: fx["init/" + k] for k in J.NAMES})  # the recording's own weights, call by call
    worst = worst_l = 0.0
    for c in range(3):
        pos = np.searchsorted(fx["rows/index"], fx["c%d/idx" % c])
        batch = tuple(fx["rows/" + k][pos] for k in names)
        bd = J.bf16_bounds(host, batch)
        done = bool(fx["c%d/done" % c])
        loss = float(tr.train_on(dev, torch.as_tensor(pos).cuda(), done=done))
        gd = {k: v.cpu() for k, v in tr.grad_dict().items()}
        worst = max(worst, J.worst_share(gd, {k: torch.as_tensor(fx["c%d/grad/%s" % (c, k)]) for k in J.NAMES}, bd))
        worst_l = max(worst_l, abs(loss - float(fx["c%d/loss" % c])) / bd["loss"])
        tsd, msd = tr.target_state_dict(), tr.state_dict()
        assert all(torch.equal(tsd[k], msd[k]) for k in J.NAMES) == bool(fx["c%d/target_eq_model" % c])
        for k in J.NAMES[:2]:  # layer1 has moved
            assert float((msd[k].cpu() != host["sd"][k]).float().mean()) > 0.99, k
        # the recording's own next weights: the device's differ from them by what one Adam step of at most about lr per
        # float can (a sign where a gradient is near zero), far inside a bfloat16 spacing of most weights
        J.fp32_train_step(host, batch)
        if done:
            J.sync_target(host)
    print("\nMEASURED the three recorded calls: worst share of the bf16 bound, gradient %.3g, loss %.3g" % (worst, worst_l))
    assert worst <= 1.0 and worst_l <= 1.0 and tr.syncs == 1
