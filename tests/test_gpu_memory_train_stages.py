"""The memory agent's training step on the device, bit for bit and stage by stage.  These are the sharp
checks of antsrl_memtrain.hip; tests/test_gpu_memory_train.py keeps the end-to-end ones (the reference's fixture, fp32
cosine, fitting a minibatch, the environment loop) at their looser, measured tolerances.

An end-to-end a-priori bound cannot be had: the contract rounds every layer's input to bf16 and masks by ReLU, so a
last-bit difference in an fp32 sum can flip a rounding or a mask downstream.  Two tests go round that from opposite sides.

test_exact_cases_bit_for_bit: inputs for which every fp32 sum of the step is exact (memory_train_cases.EXACT; the premise
is tests/test_memory_train_bounds_cpu.py), so the result depends neither on summation order nor on where the launches
are cut: the gradients, all trained_floats of them, and the loss equal float64; then three step()s at lr 2^-10, betas
(0.5, 0.5): m and v equal memory_train_ref.adam_step bit for bit, the parameters within
    2^-23 max(|p|, |p'|) + 2 gamma(16) |p' - p|
of it (both sides round the new parameter once, 2^-24 |p'| each; the update m / (sqrt(v) / c + eps) * s is five
operations, each within 3 units of roundoff of exact whether the division is correctly rounded or HIP's 2.5 ulp one),
and after every step both bf16 packs equal bf16(master), padding included, as they do in the target after sync_target()
and in both nets after load_state_dict().  Equality is of values: -0 equals +0.

test_every_launch_inside_its_bound: ordinary data (memory_train_cases.STAGE); the workspace is read back and each of the
16 launches is held, element by element, against float64 on ITS OWN inputs as the device left them, inside
gamma(K + 3) (sum |a||w| + |bias| + |residual|) + 2^-126 (K + 3) (memory_train_ref.stage_outputs).  No rounding point or
mask lies between a launch's input and its output (ReLU and max are 1-Lipschitz, the backward mask is read from the
device's own activation), so the bound is rigorous.  Padding is exactly 0.  The packs are checked here too.  The worst
share of the bound per launch is printed (-s) and recorded in profiles/memory_train_stages.json."""
import json

import pytest
import torch

import memory_train_cases as K
import memory_train_ref as R

pytestmark = pytest.mark.gpu


def _trainer(case, inp, **kw):
    """A MemoryTrainer holding inp's model and, as its target net, inp's target (load_state_dict sets both nets, so the
    target's state buffer is taken from a second trainer: the same layout, masters and packs)."""
    from antsrl_amd.train import MemoryTrainer
    tr = MemoryTrainer(case["F"], "cuda", state_dict=inp["sd"], discount=case["discount"], **kw)
    other = MemoryTrainer(case["F"], "cuda", state_dict=inp["target"])
    tr._target.copy_(other._model)
    return tr


def _dev(inp):
    arrays = tuple(t.cuda().contiguous() for t in inp["arrays"])
    return arrays, (None if inp["idx"] is None else inp["idx"].cuda().contiguous())


def _state(buf, L):
    """(params [params_floats], m, v [trained_floats]) of a state buffer, on the CPU."""
    b = buf.cpu()
    f = b.view(torch.float32)
    t = L["trained_floats"]
    return b, f[:L["params_floats"]].clone(), f[L["m_off"] // 4: L["m_off"] // 4 + t].clone(), f[L["v_off"] // 4: L["v_off"] // 4 + t].clone()


def _weights(params, L):
    return [params[L["poff"][l]: L["poff"][l] + L["out"][l] * L["inn"][l]].view(L["out"][l], L["inn"][l]) for l in range(9)]


def _assert_packs(buf, L, what):
    b, params, _, _ = _state(buf, L)
    for l, ((w, wt), (ew, ewt)) in enumerate(zip(R.read_packs(b, L), R.expected_packs(_weights(params, L), L))):
        assert torch.equal(w, ew), (what, "W", l)
        assert torch.equal(wt, ewt), (what, "W^T", l)


@pytest.mark.parametrize("case", K.EXACT, ids=K.EXACT_IDS)
def test_exact_cases_bit_for_bit(case):
    inp = K.exact_inputs(case)
    ref = K.exact_trace(case, inp)
    lr, betas = 2.0 ** -10, (0.5, 0.5)
    tr = _trainer(case, inp, lr=lr, betas=betas)
    L = R.state_layout(*K.dims(case))
    assert tr.trained_floats == L["trained_floats"] and tr.state_bytes == L["bytes"]
    arrays, idx = _dev(inp)
    loss = tr.grad(arrays, idx)
    want = K.flat(ref["grads"])
    got = tr.grads.cpu()
    assert got.numel() == want.numel() == tr.trained_floats
    bad = (got.double() != want).nonzero().view(-1)
    assert bad.numel() == 0, (bad.numel(), [(int(i), float(got[i]), float(want[i])) for i in bad[:5]])
    assert float(loss) == float(ref["loss"]), (float(loss), float(ref["loss"]))
    if idx is not None:  # idx == NULL on the gathered copy: the same bits
        again = _trainer(case, inp, lr=lr, betas=betas)
        l2 = again.grad(tuple(t[idx].contiguous() for t in arrays))
        assert torch.equal(l2, loss) and torch.equal(again.grads, tr.grads)
    _assert_packs(tr._model, L, "fresh")
    _assert_packs(tr._target, L, "fresh target")
    T = L["trained_floats"]
    for s in (1, 2, 3):
        _, p0, m0, v0 = _state(tr._model, L)
        tr.step(arrays, idx)
        g = tr.grads.cpu()
        if s == 1:
            assert torch.equal(g, got)
        ep, em, ev = R.adam_step(p0[:T], g, m0, v0, s, lr, betas[0], betas[1])
        _, p1, m1, v1 = _state(tr._model, L)
        assert torch.equal(m1, em) and torch.equal(v1, ev), s
        tol = 2.0 ** -23 * torch.maximum(p0[:T].abs(), ep.abs()).double() + 2 * R.gamma(16) * (ep.double() - p0[:T].double()).abs()
        err = (p1[:T].double() - ep.double()).abs()
        assert bool((err <= tol).all()), (s, float((err / tol.clamp(min=1e-300)).max()))
        assert torch.equal(p1[T:], p0[T:])  # the memory head
        assert bool((p1[:T] != p0[:T]).any())
        _assert_packs(tr._model, L, "step %d" % s)
    tr.sync_target()
    assert torch.equal(tr._target.cpu()[:L["params_floats"] * 4], tr._model.cpu()[:L["params_floats"] * 4])
    _assert_packs(tr._target, L, "after sync_target")
    _, _, m3, v3 = _state(tr._model, L)
    tr.load_state_dict(inp["target"])
    _assert_packs(tr._model, L, "after load_state_dict")
    _assert_packs(tr._target, L, "target after load_state_dict")
    _, p4, m4, v4 = _state(tr._model, L)
    assert torch.equal(m4, m3) and torch.equal(v4, v3)  # Adam's state is kept
    assert torch.equal(_weights(p4, L)[0], inp["target"]["layer1.weight"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", K.STAGE, ids=K.STAGE_IDS)
def test_every_launch_inside_its_bound(case):
    inp = K.stage_inputs(case)
    tr = _trainer(case, inp, lr=1e-4)
    W = R.work_layout(*K.dims(case), case["B"])
    L = W["L"]
    arrays, idx = _dev(inp)
    loss = tr.grad(arrays, idx)
    assert tr._work.numel() >= W["bytes"]
    work = tr._work.cpu().view(torch.float32)
    img = R.read_workspace(work, W)
    img["grads"], img["loss"] = tr.grads.cpu(), loss.cpu()
    model = {k: v.cpu() for k, v in tr.state_dict().items()}
    target = {k: v.cpu() for k, v in tr.target_state_dict().items()}
    assert all(torch.equal(model[k], inp["sd"][k]) and torch.equal(target[k], inp["target"][k]) for k in model)
    P = R.problem(model, target, inp["arrays"], inp["idx"], case["B"], case["discount"], K.dims(case))
    shares = {s: R.check_stage(s, img, P) for s in R.STAGES}
    print("\nSTAGE-GPU-SHARE %s" % json.dumps({"case": case["name"], "shares": {s: round(v, 4) for s, v in shares.items()}}))
    assert max(shares.values()) <= 1.0, shares
    assert bool(torch.isfinite(img["grads"]).all()) and bool(torch.isfinite(img["loss"]))
    # the packs: bf16(master) in both nets, after a step of lr 1e-4 (below a bf16 ulp of most weights), in the target
    # after the sync, and in both after a load
    _assert_packs(tr._model, L, "fresh")
    _assert_packs(tr._target, L, "fresh target")
    before = tr._model.cpu()
    tr.apply()
    assert not torch.equal(before[:L["trained_floats"] * 4], tr._model.cpu()[:L["trained_floats"] * 4])
    _assert_packs(tr._model, L, "after apply")
    tr.sync_target()
    assert torch.equal(tr._target.cpu()[:L["params_floats"] * 4], tr._model.cpu()[:L["params_floats"] * 4])
    _assert_packs(tr._target, L, "after sync_target")
    tr.load_state_dict(inp["target"])
    _assert_packs(tr._model, L, "after load_state_dict")
    _assert_packs(tr._target, L, "target after load_state_dict")
    torch.cuda.synchronize()
