"""The bounds the GPU tests of antsrl_jointtrain_step rest on (tests/joint_train_ref.py), checked without a GPU:
contract_train_step stays within bf16_bounds of the torch autograd step, two fp32 restatements of the contract in
different summation orders stay inside fp32_sum_bounds (SAFE), and each of eight defects a device could have leaves that
bound on at least one element at every case (SHARP); the same per workgroup of the forward stage
(joint_train_ref.partial_bounds of expected_partials).  -s prints the worst share of each bound.

That every defect can be told apart at every case is a condition on the inputs (joint_train_ref.make_case: signed
observations with bfloat16 ties, agent states that round, rewards that leave both heads TD errors of the size of their q,
some rows done and some not), checked here before any device run."""
import ctypes as C

import numpy as np
import pytest
import torch

import joint_train_ref as J

DEFECTS = ("dh_without_pheromone_term", "dh_w3_row_of_rotation_action", "stale_w1_for_h_next", "model_layer3_for_target",
           "agent_columns_dropped", "no_g_b1", "dones_ignored", "scale_2_over_B")
#: the defects that reach the forward stage's partials (the heads' gradients and the loss)
PARTIAL_DEFECTS = ("stale_w1_for_h_next", "model_layer3_for_target", "dones_ignored", "scale_2_over_B")


def _rowsum(terms, order):
    """terms [B, ...] fp32 -> the sum over rows in fp32: "torch" (torch's own order), or "device": rows w, w + 16, ... per
    wave in ascending order, then the 16 waves in order from wave 0's (dqn_l1_stage)."""
    if order == "torch":
        return terms.sum(0)
    B = terms.shape[0]
    pad = torch.zeros((-(-B // 16) * 16,) + terms.shape[1:], dtype=torch.float32)
    pad[:B] = terms
    pad = pad.view((-1, 16) + terms.shape[1:])  # [step][wave]: a row beyond B adds +0, which changes no sum from zero
    acc = torch.zeros_like(pad[0])
    for s in range(pad.shape[0]):
        acc = acc + pad[s]
    total = acc[0]
    for w in range(1, 16):
        total = total + acc[w]
    return total


def stale(w1):
    """A copy of W1 that lags by two bfloat16 spacings per weight: the smallest staleness every weight's bfloat16 image
    shows (an Adam step at lr 1e-4 is below one spacing for most weights, and is by contract invisible until it adds up)."""
    return w1 * (1.0 + 2.0 ** -6)


def restate_fp32(state, batch, discount, order, defect=None):
    """The contract with every sum taken in fp32 in the given order (and optionally one defect)."""
    st, ast, act, rw, nst, nast, dn = J._clamped(batch)
    sd = state["sd"]
    B, F = st.shape

    def hidden(w1, x, a):
        xe, w = J.bf16(torch.cat([x, a], 1)), J.bf16(w1)
        if order == "torch":
            return xe, xe @ w.T + sd[J.B1]
        return xe, (xe.flip(1) @ w.flip(1).T) + sd[J.B1]
    xe, h = hidden(sd[J.W1], st, ast)
    _, hn = hidden(stale(sd[J.W1]) if defect == "stale_w1_for_h_next" else sd[J.W1], nst, nast)
    tw3, tb3 = (sd[J.W3], sd[J.B3]) if defect == "model_layer3_for_target" else (state["target_w3"], state["target_b3"])
    qr, qp = h @ sd[J.W2].T + sd[J.B2], h @ sd[J.W3].T + sd[J.B3]
    nr, npq = hn @ sd[J.W2].T + sd[J.B2], hn @ tw3.T + tb3
    live = torch.ones_like(rw) if defect == "dones_ignored" else (~dn).to(torch.float32)
    rows = torch.arange(B)
    ar, ap = act[:, 0], act[:, 1]
    dr = qr[rows, ar] - (rw + discount * nr.max(dim=1).values * live)
    dp = qp[rows, ap] - (rw + discount * npq.max(dim=1).values * live)
    scale = float(np.float32((2.0 / B) if defect == "scale_2_over_B" else 2.0 / (3.0 * B)))
    gr, gp = dr * scale, dp * scale
    dq = torch.zeros((B, 6))
    dq[rows, ar] = gr
    dq[rows, 3 + ap] = gp
    if defect == "dh_without_pheromone_term":
        dh = gr[:, None] * sd[J.W2][ar]
    else:
        dh = gr[:, None] * sd[J.W2][ar] + gp[:, None] * sd[J.W3][ar if defect == "dh_w3_row_of_rotation_action" else ap]
    if B <= 600:
        gw1 = _rowsum(dh[:, :, None] * xe[:, None, :], order)
        gwh = _rowsum(dq[:, :, None] * h[:, None, :], order)
    else:  # (the outer products of thousands of rows at once are large: torch's fp32 matmul, rows reversed for the second order)
        o = slice(None) if order == "torch" else torch.arange(B - 1, -1, -1)
        gw1, gwh = dh[o].T @ xe[o], dq[o].T @ h[o]
    gbh = _rowsum(dq, order)
    grads = {J.W1: gw1, J.B1: _rowsum(dh, order), J.W2: gwh[:3], J.B2: gbh[:3], J.W3: gwh[3:], J.B3: gbh[3:]}
    if defect == "agent_columns_dropped":
        grads[J.W1] = grads[J.W1].clone()
        grads[J.W1][:, F:] = 0.0
    if defect == "no_g_b1":
        grads[J.B1] = torch.zeros((32,))
    inv = float(np.float32(1.0 / (3.0 * B)))
    lterm = dr * dr * inv + dp * dp * inv
    loss = float(_rowsum(lterm, order))
    # the forward stage's partials: a workgroup's 128 rows in torch's order, or tile by tile, wave by wave in the device's
    terms = J.row_terms(torch.cat([dq, lterm[:, None]], 1), h)
    if order == "torch":
        part = torch.stack([terms[g:g + 128].sum(0) for g in range(0, B, 128)])
    else:
        total, part = J.device_order_sum(terms, B)  # tile / wave / workgroup order: the heads' gradients and the loss
        loss = float(total[198])
        grads[J.W2], grads[J.B2] = total[0:96].view(3, 32), total[96:99]
        grads[J.W3], grads[J.B3] = total[99:195].view(3, 32), total[195:198]
    return loss, grads, dict(act=act, dn=dn, part=part)


def _cases():
    for F, B in J.SHAPES:
        state, arrays, idx = J.shape_case(F, B)
        yield "F%d_B%d" % (F, B), state, J.gather(arrays, idx), 0.5


CASES = list(_cases())
IDS = [c[0] for c in CASES]


def _variants():
    for name in J.VARIANTS:
        state, arrays, idx, discount, B = J.make_variant(name)
        yield name, state, J.gather_clamped(arrays, idx, B), discount


VCASES = CASES + list(_variants())
VIDS = [c[0] for c in VCASES]


@pytest.mark.parametrize("name,state,batch,discount", VCASES, ids=VIDS)
def test_the_contract_stays_within_the_bf16_bound_of_autograd(name, state, batch, discount):
    loss_c, g_c = J.contract_train_step(state, batch, discount, update=False)
    loss_f, g_f = J.fp32_train_step(state, batch, discount, update=False)
    bd = J.bf16_bounds(state, batch, discount)
    # the fp32 side sums in fp32: its own summation error, bounded by fp32_sum_bounds, comes on top
    fs = J.fp32_sum_bounds(state, batch, discount)
    both = {k: torch.as_tensor(bd[k]) + torch.as_tensor(fs[k]) for k in J.NAMES}
    share = J.worst_share(g_c, g_f, both)
    share_l = abs(loss_c - loss_f) / (bd["loss"] + fs["loss"]) if loss_c != loss_f else 0.0
    print("\n%-16s bf16 bound: gradient share %.3g, loss share %.3g" % (name, share, share_l))
    assert share <= 1.0 and share_l <= 1.0


@pytest.mark.parametrize("name,state,batch,discount", VCASES, ids=VIDS)
def test_safe_two_fp32_orders_use_a_small_share_of_the_sum_bound(name, state, batch, discount):
    loss_c, g_c = J.contract_train_step(state, batch, discount, update=False)
    bd = J.fp32_sum_bounds(state, batch, discount)
    worst = 0.0
    for order in ("torch", "device"):
        loss, g, _ = restate_fp32(state, batch, discount, order)
        share, share_l = J.worst_share(g, g_c, bd), (abs(loss - loss_c) / bd["loss"] if loss != loss_c else 0.0)
        worst = max(worst, share, share_l)
        assert share <= 1.0 and share_l <= 1.0, (order, share, share_l)
    print("\n%-16s fp32 sum bound: clean restatements use %.3g of it" % (name, worst))
    assert worst <= 0.5  # a small share: the bound is not so loose that it hides a defect


@pytest.mark.parametrize("name,state,batch,discount", CASES, ids=IDS)
def test_sharp_every_defect_leaves_the_sum_bound(name, state, batch, discount):
    """At every shape (discount 0.5; make_case puts a live row with two different actions and, from two rows on, a done
    row into the batch) every defect must show.  A batch of ONE row is live, so ignoring dones changes nothing there:
    that is the one defect and the one case left out, by this reasoning and not by a measurement."""
    loss_c, g_c = J.contract_train_step(state, batch, discount, update=False)
    bd = J.fp32_sum_bounds(state, batch, discount)
    _, _, info = restate_fp32(state, batch, discount, "torch")
    act, dn = info["act"], info["dn"]
    B = len(dn)
    assert bool((act[:, 0] != act[:, 1]).any()) and not bool(dn.all()) and (B == 1 or bool(dn.any()))  # the inputs' part
    cannot = {"dones_ignored"} if B == 1 else set()
    least = float("inf")
    for defect in DEFECTS:
        if defect in cannot:
            continue
        loss, g, _ = restate_fp32(state, batch, discount, "torch", defect)
        share = max(J.worst_share(g, g_c, bd), abs(loss - loss_c) / bd["loss"])
        least = min(least, share)
        assert share > 1.0, (defect, share)
    print("\n%-16s fp32 sum bound: the mildest defect stands %.3g x outside (%d of %d defects can show)"
          % (name, least, len(DEFECTS) - len(cannot), len(DEFECTS)))


# ---- the forward stage's partials and the workspace ---------------------------------------------------------------------
def _partial_share(part, want, bound):
    err = (part.double() - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


@pytest.mark.parametrize("F,B", J.SHAPES)
def test_the_workspace_layout_is_the_librarys(F, B):
    from antsrl_amd import _lib
    from antsrl_amd import build as buildmod
    buildmod.build_hip()
    ws = C.c_size_t()
    assert _lib.load().antsrl_jointtrain_sizes(F, B, None, C.byref(ws), None) == 0
    W = J.work_layout(B)
    assert ws.value == W["bytes"] == W["dh_offset"] + 128 * B
    assert W["dh_offset"] % 256 == 0 and 0 <= W["dh_offset"] - W["blocks"] * J.PART * 4 < 256
    assert W["blocks"] == -(-(-(-B // 32)) // 4) == int(J.row_workgroup(B).max()) + 1


def test_the_lds_seam_lies_between_608_and_609():
    assert J.lds_bytes(608) <= 65536 < J.lds_bytes(609) and J.lds_bytes(1022) <= 160 * 1024


@pytest.mark.parametrize("name,state,batch,discount", CASES, ids=IDS)
def test_fp32_partials_stay_inside_the_per_partial_bound_and_every_defect_leaves_it(name, state, batch, discount):
    B = len(batch[3])
    want, bound = J.expected_partials(state, batch), J.partial_bounds(state, batch)
    loss_c, g_c = J.contract_train_step(state, batch, update=False)
    flat = torch.cat([g_c[J.W2].reshape(-1), g_c[J.B2], g_c[J.W3].reshape(-1), g_c[J.B3], torch.tensor([loss_c])]).double()
    assert bool(((want.sum(0) - flat).abs() <= 2.0 ** -22 * want.abs().sum(0)).all())  # the contract's sums, cut by workgroup
    worst = 0.0
    for order in ("torch", "device"):
        part = restate_fp32(state, batch, 0.5, order)[2]["part"]
        assert part.shape == want.shape == bound.shape == (J.blocks(B), J.OUT)
        worst = max(worst, _partial_share(part, want, bound))
    assert worst <= 1.0, worst
    least = float("inf")
    for defect in PARTIAL_DEFECTS:
        if B == 1 and defect != "scale_2_over_B":
            continue
        share = _partial_share(restate_fp32(state, batch, 0.5, "device", defect)[2]["part"], want, bound)
        least = min(least, share)
        assert share > 1.0, (defect, share)
    print("\n%-16s per-partial bound: clean restatements use %.3g of it, the mildest defect %.3g x" % (name, worst, least))
