"""The rework agent's training step on the device (antsrl_reworktrain_*, ReworkTrainer), stage by stage
against tests/rework_train_ref.py:

 1. the down chain: the model's collapsed buffer is rework_policy_ref.collapse64's in every bit, every M_l down_chain's;
 2. the partials: their ordered fp32 sum is G, s and (each head's scale applied once) the loss, in every bit;
 3. the up chain and the gradient: from the device's own G and s, `contract` gives every A_l and all 20 gradients in every bit;
 4. accuracy: per tensor max |g - g64| <= 4 max(e_ref, floor) and the loss likewise (accuracy_bounds: nothing of the bound
    comes from the device);
 5. step() holds the bits of grad() then apply(); keep_grads=False leaves the gradient buffer alone; twins and a second
    grad() agree in every bit;
 6. Adam from the device's own gradient: the moments bit for bit, the parameters within agent_harness.param_tolerance;
 7. guards around the workspace, gradients, loss, the model block, Adam's state and the target's collapsed buffer stay
    intact, the target block is not touched, and a zeroed workspace gives the bits of one filled with 0xFF;
 8. the reference's three recorded train() calls through train_on;
 9. acting: a step moves neither policy.act's q nor `version`; after sync_target the policy equals a fresh ReworkPolicy.

The cases are rework_train_ref.CASES and VARIANTS: the smallest shapes at which each seam of the kernels exists."""
import functools

import numpy as np
import pytest
import torch

import rework_policy_ref as R
import rework_train_ref as T
from agent_harness import param_tolerance, same_bits

pytestmark = pytest.mark.gpu

GUARD = 4096
ALL = tuple(T.CASES) + T.VARIANTS


@functools.lru_cache(maxsize=None)
def _host(name):
    """(state, arrays, idx or None, B) on the CPU, and the gathered batch."""
    if name in T.CASES:
        state, arrays, idx = T.case(name)
        B = len(idx)
    else:
        state, arrays, idx, B = T.make_variant(name)
    return state, arrays, idx, B, T.gather_clamped(arrays, idx, B)


def _trainer(state, **kw):
    """A ReworkTrainer holding state's model and its (different) target."""
    from antsrl_amd.train import ReworkTrainer
    F = state["sd"]["layer1.weight"].shape[1] - 2
    tr = ReworkTrainer(F, "cuda", state_dict=state["sd"], **kw)
    tr.target.copy_(torch.cat([state["target"][k].reshape(-1) for k in T.NAMES]))
    tr.policy.recollapse()
    return tr


def _dev(arrays, idx):
    return tuple(t.cuda() for t in arrays), (None if idx is None else idx.cuda())


def _bits64(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _snapshot(tr, loss, sd, B):
    ws = T.read_workspace(tr._work.cpu(), sd, B)
    s = dict(loss=loss.detach().cpu().reshape(1), grads=tr.grads.cpu(), model=tr.model.cpu(), adam=tr._adam.cpu().reshape(-1),
             Wc=ws["Wc"].reshape(-1), bc=ws["bc"], G=ws["G"].reshape(-1), s=ws["s"], partials=ws["partials"].reshape(-1))
    for l in T.LAYERS:
        s["M/" + l] = ws["M"][l].view(torch.float32).reshape(-1)
    for l in T.A_LAYERS:
        s["A/" + l] = ws["A"][l].view(torch.float32).reshape(-1)
    return s


@pytest.mark.parametrize("name", ALL)
def test_stages_bit_for_bit_and_the_gradient_within_its_bound(name):
    state, arrays, idx, B, batch = _host(name)
    sd = state["sd"]
    n_rot, n_ph = T.heads(sd)
    NQ, Dm = n_rot + n_ph, sd["layer1.weight"].shape[1]
    tr = _trainer(state)
    darr, didx = _dev(arrays, idx)
    loss = tr.grad(darr, didx)
    torch.cuda.synchronize()
    assert tr.launches(B) == 4
    ws = T.read_workspace(tr._work.cpu(), sd, B)
    # 1. the down chain
    wc, bc = R.collapse64(sd)
    assert same_bits(ws["Wc"], wc) and same_bits(ws["bc"], bc)
    M = T.down_chain(sd)
    for l in T.LAYERS:
        assert _bits64(ws["M"][l], torch.from_numpy(M[l])), l
    # 2. the partials
    total = T.ordered_sum(ws["partials"])
    assert same_bits(total[: NQ * Dm].view(NQ, Dm), ws["G"]) and same_bits(total[NQ * Dm: NQ * Dm + NQ], ws["s"])
    lsum = total[NQ * Dm + NQ:].numpy()
    want = lsum[0] * np.float32(1.0 / (n_rot * B)) + lsum[1] * np.float32(1.0 / (n_ph * B))
    assert want.dtype == np.float32 and same_bits(loss.cpu().reshape(1), torch.from_numpy(np.array([want])))
    # 3. the up chain and the gradient, from the device's own G and s
    A, grads = T.contract(sd, ws["G"].numpy(), ws["s"].numpy(), M)
    for l in T.A_LAYERS:
        assert _bits64(ws["A"][l], torch.from_numpy(A[l])), l
    got = {k: v.cpu() for k, v in tr.grad_dict().items()}
    for k in T.NAMES:
        assert same_bits(got[k], grads[k]), k
    # 4. accuracy
    bd, g64, l64 = T.accuracy_bounds(state, batch)
    e = T.tensor_errors(got, g64)
    share = max(e[k] / bd[k] for k in T.NAMES)
    units = max(e[k] / (T.U_FP32 * float(g64[k].abs().max())) for k in T.NAMES)
    print("\nMEASURED %-18s gradient: %.3g of its bound (worst tensor %.3g x 2^-24 of its largest); loss %.3g of its bound"
          % (name, share, units, abs(float(loss) - l64) / bd["loss"]))
    for k in T.NAMES:
        assert e[k] <= bd[k], (k, e[k], bd[k])
    assert abs(float(loss) - l64) <= bd["loss"], (float(loss), l64, bd["loss"])


PATH_CASES = ("F9_B5", "F294_B264", "F1022_B5_h18", "F9_B4113", "idx_null")


@pytest.mark.parametrize("name", PATH_CASES)
def test_step_is_grad_then_apply_and_twins_agree(name):
    state, arrays, idx, B, batch = _host(name)
    darr, didx = _dev(arrays, idx)
    a, b, c = _trainer(state, lr=1e-3), _trainer(state, lr=1e-3), _trainer(state, lr=1e-3)
    la = a.step(darr, didx)
    lb = b.grad(darr, didx)
    first = _snapshot(b, lb, state["sd"], B)
    lb2 = b.grad(darr, didx)
    again = _snapshot(b, lb2, state["sd"], B)
    for k in first:
        assert same_bits(first[k], again[k]), ("a second grad()", k)
    b.apply()
    c.grads.fill_(7.0)
    lc = c.step(darr, didx, keep_grads=False)
    torch.cuda.synchronize()
    assert bool((c.grads == 7.0).all())
    sa, sb, sc = _snapshot(a, la, state["sd"], B), _snapshot(b, lb, state["sd"], B), _snapshot(c, lc, state["sd"], B)
    for k in sa:
        assert same_bits(sa[k], sb[k]), ("step against grad then apply", k)
        if k != "grads":
            assert same_bits(sa[k], sc[k]), ("keep_grads=False", k)
    assert not torch.equal(a.model, a.target) and a.step_count == b.step_count == 1
    # 6. Adam from the device's own gradient
    host = T.new_state(state["sd"], state["target"])
    before = {k: v.clone() for k, v in host["sd"].items()}
    T.adam(host, {k: v.cpu() for k, v in a.grad_dict().items()}, lr=1e-3)
    st, after = a.adam_state(), a.state_dict()
    for k in T.NAMES:
        assert torch.equal(st["exp_avg"][k].cpu(), host["m"][k]) and torch.equal(st["exp_avg_sq"][k].cpu(), host["v"][k]), k
        assert ((after[k].cpu() - host["sd"][k]).abs() <= param_tolerance(host["sd"][k], before[k])).all(), k
    assert any(not torch.equal(after[k].cpu(), before[k]) for k in T.NAMES)


def _guarded_copy(t, byte):
    """(buffer, offset, bytes, a 256-byte aligned tensor of t's shape, dtype and content between two guards of `byte`)."""
    n = t.numel() * t.element_size()
    buf = torch.full((n + 2 * GUARD + 256,), byte, dtype=torch.uint8, device="cuda")
    off = GUARD + (-(buf.data_ptr() + GUARD)) % 256
    view = buf[off: off + n].view(t.dtype).view(t.shape)
    view.copy_(t)
    return buf, off, n, view


@pytest.mark.parametrize("name", ("F9_B17_h18", "F294_B33_odd_h25", "F1022_B17", "idx_clamped"))
@pytest.mark.parametrize("mode", ("grad", "step"))
def test_writes_stay_inside_and_nothing_is_read_before_it_is_written(name, mode):
    state, arrays, idx, B, batch = _host(name)
    darr, didx = _dev(arrays, idx)
    runs = []
    for fill in (0x00, 0xFF):
        tr = _trainer(state)
        nbytes = T.work_layout(state["sd"], B)["bytes"]
        target_before = tr.target.clone()
        held = {}
        for what, t in (("model", tr.model), ("adam", tr._adam), ("grads", tr.grads), ("collapsed", tr.policy.collapsed),
                        ("loss", torch.zeros((), device="cuda")), ("work", torch.zeros((nbytes,), dtype=torch.uint8, device="cuda"))):
            held[what] = _guarded_copy(t, 0xA5)
        tr.model, tr._adam, tr.grads, tr.policy.collapsed, loss, tr._work = (held[k][3] for k in ("model", "adam", "grads", "collapsed", "loss", "work"))
        tr._work.fill_(fill)
        tr.grads.view(torch.uint8).fill_(fill)
        loss.reshape(1).view(torch.uint8).fill_(fill)
        out = tr.grad(darr, didx, loss=loss) if mode == "grad" else tr.step(darr, didx, loss=loss)
        torch.cuda.synchronize()
        assert out is loss and tr._work.data_ptr() == held["work"][3].data_ptr()
        for what, (buf, off, n, _) in held.items():
            host = buf.cpu()
            assert bool((host[:off] == 0xA5).all()) and bool((host[off + n:] == 0xA5).all()), (what, fill, "guards")
        assert torch.equal(tr.target, target_before)
        runs.append(_snapshot(tr, loss, state["sd"], B))
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), ("zero bytes against 0xFF bytes", k)


def test_the_references_three_calls():
    """train_on with the recorded idx and done: the losses within the loss bound of the recorded ones, the target equal to
    the model after the done call only, the final parameters within the CPU test's tolerance (test_rework_train_fixture.
    reference_run) of the reference's."""
    from test_rework_train_fixture import CALLS, FIXTURE, RECORDED, fixture_arrays, reference_run
    z = np.load(FIXTURE)
    arrays, idx = fixture_arrays(z)
    darr, _ = _dev(arrays, None)
    host = T.new_state(R.load_model("init")[0])
    tr = _trainer(host)
    assert tr.discount == 0.5 and tr.lr == 1e-4 and tr.minibatch == 264 and tr.update_target_every == 1
    for c in range(CALLS):
        batch = T.gather(arrays, idx[c])
        bd, _, l64 = T.accuracy_bounds(host, batch)
        done = bool(z["c%d/done" % c])
        loss = float(tr.train_on(darr, idx[c].cuda(), done))
        print("\nMEASURED call %d: loss %.9g, recorded %.9g, float64 %.9g, bound %.3g" % (c, loss, float(z["c%d/loss" % c]), l64, bd["loss"]))
        assert abs(loss - float(z["c%d/loss" % c])) <= bd["loss"]
        assert torch.equal(tr.model, tr.target) == done
        T.fp32_train_step(host, batch)  # (the bound of the next call's loss is taken at the reference's parameters)
        if done:
            T.sync_target(host)
    assert tr.syncs == 1 and tr.step_count == 3
    ref, tol, _ = reference_run(z)
    after = tr.state_dict()
    worst = max(float(((after[k].cpu() - ref[k]).abs() / tol[k]).max()) for k in RECORDED)
    print("MEASURED final parameters: %.3g of their tolerance" % worst)
    for k in RECORDED:
        assert ((after[k].cpu() - ref[k]).abs() <= tol[k]).all(), k


def test_a_step_does_not_move_the_acting_net_and_a_sync_does():
    from antsrl_amd.policy import ReworkPolicy
    state, arrays, idx, B, batch = _host("F294_B264")
    darr, didx = _dev(arrays, idx)
    tr = _trainer(state, lr=1e-2)
    obs = darr[0][:64].reshape(64, 7, 7, 6).contiguous()
    ast = darr[1][:64].contiguous()

    def q():
        out = torch.empty((64, 6), device="cuda")
        rot, ph = tr.policy.act(obs, ast, logits=out)
        return out.clone(), rot.clone(), ph.clone()
    q0, v0, col0 = q(), tr.version, tr.policy.collapsed.clone()
    tr.step(darr, didx)
    q1 = q()
    assert tr.version == v0 and same_bits(col0, tr.policy.collapsed) and all(same_bits(a.float(), b.float()) for a, b in zip(q0, q1))
    tr.sync_target()
    assert tr.version == v0 + 1 and torch.equal(tr.model, tr.target)
    fresh = ReworkPolicy(294, "cuda")
    fresh.load_state_dict(tr.target_state_dict())
    assert same_bits(fresh.collapsed, tr.policy.collapsed) and not same_bits(col0, tr.policy.collapsed)
    out = torch.empty((64, 6), device="cuda")
    rot, ph = fresh.act(obs, ast, logits=out)
    q2 = q()
    assert same_bits(out, q2[0]) and torch.equal(rot, q2[1]) and torch.equal(ph, q2[2])
    assert all(v.data_ptr() == w.data_ptr() for v, w in zip(tr.policy.params.values(), tr._views(tr.target).values()))
