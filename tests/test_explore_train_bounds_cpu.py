"""The bounds the GPU tests of antsrl_exptrain_step rest on (tests/explore_train_ref.py), checked without a GPU:
contract_train_step stays within bf16_bounds of the torch autograd step, two fp32 restatements of the contract in
different row orders stay inside fp32_sum_bounds, and each of six defects a device could have leaves that bound at every
case where it can bite; the same per workgroup of the forward stage (explore_train_ref.partial_bounds of
expected_partials, at WORKSPACE_SHAPES, with the defect tile_to_wrong_workgroup on top).  -s prints the worst share of
each bound."""
import numpy as np
import pytest
import torch

import explore_train_ref as X

DEFECTS = ("target_h_from_model", "agent_columns_dropped", "no_g_b1", "dh_from_row_0", "dones_ignored", "scale_2_over_B")
#: the defects that reach the forward stage's partials (layer2's gradients and the loss), and one that reaches nothing else
PARTIAL_DEFECTS = ("target_h_from_model", "dones_ignored", "scale_2_over_B", "tile_to_wrong_workgroup")


def _rowsum(terms, order):
    """terms [B, ...] fp32 -> the sum over rows in fp32: "torch" (torch's own order), or "device": rows w, w + 16, ... per
    wave in ascending order, then the 16 waves in order (antsrl_exptrain.hip, stage 2)."""
    if order == "torch":
        return terms.sum(0)
    parts = []
    for w in range(16):
        acc = torch.zeros_like(terms[0])
        for b in range(w, terms.shape[0], 16):
            acc = acc + terms[b]
        parts.append(acc)
    total = parts[0]
    for part in parts[1:]:
        total = total + part
    return total


def restate_fp32(state, batch, discount, order, defect=None):
    """The contract with every sum taken in fp32 in the given order (and optionally one defect)."""
    st, ast, act, rw, nst, nast, dn = X._t(batch)
    sd, tg = state["sd"], state["target"]
    B, F = st.shape

    def hidden(w, x, a):
        xe = X.bf16(torch.cat([x, a], 1))
        w1 = X.bf16(w[X.W1])
        if order == "torch":
            return xe, xe @ w1.T + w[X.B1]
        return xe, (xe.flip(1) @ w1.flip(1).T) + w[X.B1]
    xe, h = hidden(sd, st, ast)
    _, hn = hidden(sd if defect == "target_h_from_model" else tg, nst, nast)
    q, qn = h @ sd[X.W2].T + sd[X.B2], hn @ tg[X.W2].T + tg[X.B2]
    a = act[:, 0].clamp(0, 2)
    live = torch.ones_like(rw) if defect == "dones_ignored" else (~dn).to(torch.float32)
    d = q[torch.arange(B), a] - (rw + discount * qn.max(dim=1).values * live)
    scale = float(np.float32((2.0 / B) if defect == "scale_2_over_B" else 2.0 / (3.0 * B)))
    g = d * scale
    dq = torch.zeros((B, 3))
    dq[torch.arange(B), a] = g
    dh = g[:, None] * sd[X.W2][torch.zeros_like(a) if defect == "dh_from_row_0" else a]
    if B <= 600:
        gw1 = _rowsum(dh[:, :, None] * xe[:, None, :], order)
        gw2 = _rowsum(dq[:, :, None] * h[:, None, :], order)
    else:  # (the outer products of 4096 rows at once are large: torch's fp32 matmul, rows reversed for the second order)
        o = slice(None) if order == "torch" else torch.arange(B - 1, -1, -1)
        gw1, gw2 = dh[o].T @ xe[o], dq[o].T @ h[o]
    grads = {X.W1: gw1, X.B1: _rowsum(dh, order), X.W2: gw2, X.B2: _rowsum(dq, order)}
    if defect == "agent_columns_dropped":
        grads[X.W1][:, F:] = 0.0
    if defect == "no_g_b1":
        grads[X.B1] = torch.zeros((32,))
    lterm = d * d * float(np.float32(1.0 / (3.0 * B)))
    loss = float(_rowsum(lterm, order))
    # the forward stage's partials: a workgroup's 128 rows in torch's order, or tile by tile in the device's
    terms = X.row_terms(torch.cat([dq, lterm[:, None]], 1), h)
    if defect == "tile_to_wrong_workgroup":  # tiles 0 and 4 change places: the first tiles of workgroups 0 and 1
        terms = torch.cat([terms[128:160], terms[32:128], terms[0:32], terms[160:]])
    if order == "torch":
        part = torch.stack([terms[g:g + 128].sum(0) for g in range(0, B, 128)])
    else:
        part = X.device_order_sum(terms, B)[1]
    return loss, grads, dict(a=a, dn=dn, d=d, part=part)


def _cases():
    for F, B in X.SHAPES:
        state, arrays, idx = X.make_case(F, B, 100 * F + B)
        yield "F%d_B%d" % (F, B), state, X.gather(arrays, idx), 0.5
    for name in X.VARIANTS:
        state, arrays, idx, discount, B = X.make_variant(name)
        yield name, state, X.gather_clamped(arrays, idx, B), discount


CASES = list(_cases())
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name,state,batch,discount", CASES, ids=IDS)
def test_the_contract_stays_within_the_bf16_bound_of_autograd(name, state, batch, discount):
    loss_c, g_c = X.contract_train_step(state, batch, discount, update=False)
    loss_f, g_f = X.fp32_train_step(state, batch, discount, update=False)
    bd = X.bf16_bounds(state, batch, discount)
    # the fp32 side sums in fp32: its own summation error, bounded by fp32_sum_bounds, comes on top
    fs = X.fp32_sum_bounds(state, batch, discount)
    both = {k: torch.as_tensor(bd[k]) + torch.as_tensor(fs[k]) for k in X.NAMES}
    share = X.worst_share(g_c, g_f, both)
    share_l = abs(loss_c - loss_f) / (bd["loss"] + fs["loss"]) if loss_c != loss_f else 0.0
    print("\n%-16s bf16 bound: gradient share %.3g, loss share %.3g" % (name, share, share_l))
    assert share <= 1.0 and share_l <= 1.0


@pytest.mark.parametrize("name,state,batch,discount", CASES, ids=IDS)
def test_two_fp32_orders_stay_inside_the_sum_bound_and_every_defect_leaves_it(name, state, batch, discount):
    loss_c, g_c = X.contract_train_step(state, batch, discount, update=False)
    bd = X.fp32_sum_bounds(state, batch, discount)
    worst = 0.0
    for order in ("torch", "device"):
        loss, g, info = restate_fp32(state, batch, discount, order)
        share, share_l = X.worst_share(g, g_c, bd), (abs(loss - loss_c) / bd["loss"] if loss != loss_c else 0.0)
        worst = max(worst, share, share_l)
        assert share <= 1.0 and share_l <= 1.0, (order, share, share_l)
    a, dn = info["a"], info["dn"]
    bites = {"target_h_from_model": discount != 0 and not bool(dn.all()), "agent_columns_dropped": True, "no_g_b1": True,
             "dh_from_row_0": bool((a != 0).any()), "dones_ignored": discount != 0 and bool(dn.any()), "scale_2_over_B": True}
    least = float("inf")
    for defect in DEFECTS:
        if not bites[defect]:
            continue
        loss, g, _ = restate_fp32(state, batch, discount, "torch", defect)
        share = max(X.worst_share(g, g_c, bd), abs(loss - loss_c) / bd["loss"])
        least = min(least, share)
        assert share > 1.0, (defect, share)
    print("\n%-16s fp32 sum bound: clean restatements use %.3g of it, the mildest defect %.3g x" % (name, worst, least))
    assert worst <= 0.5  # the clean restatements use a small share: the bound is not so loose that it hides a defect


# ---- the forward stage's partials: what test_gpu_dqn_train_workspace.py reads back from the workspace ------------------
def _partial_share(part, want, bound):
    """The largest |partial - expected| / bound over [workgroup][output] (0 / 0 = 0; an error over a zero bound = inf)."""
    err = (part.double() - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


@pytest.mark.parametrize("F,B", X.WORKSPACE_SHAPES)
def test_the_workspace_layout_is_the_librarys(F, B):
    import ctypes as C
    from antsrl_amd import _lib
    from antsrl_amd import build as buildmod
    buildmod.build_hip()
    ws = C.c_size_t()
    assert _lib.load().antsrl_exptrain_sizes(F, B, None, C.byref(ws), None) == 0
    W = X.work_layout(B)
    assert ws.value == W["bytes"] == W["dh_offset"] + 128 * B
    assert W["dh_offset"] % 256 == 0 and 0 <= W["dh_offset"] - W["blocks"] * X.PART * 4 < 256
    assert W["blocks"] == -(-(-(-B // 32)) // 4) == int(X.row_workgroup(B).max()) + 1


@pytest.mark.parametrize("F,B", X.WORKSPACE_SHAPES)
def test_fp32_partials_stay_inside_the_per_partial_bound_and_every_defect_leaves_it(F, B):
    state, arrays, idx = X.workspace_case(F, B)
    batch = X.gather(arrays, idx)
    want, bound = X.expected_partials(state, batch), X.partial_bounds(state, batch)
    loss_c, g_c = X.contract_train_step(state, batch, update=False)
    flat = torch.cat([g_c[X.W2].reshape(-1).double(), g_c[X.B2].double(), torch.tensor([loss_c], dtype=torch.float64)])
    assert bool(((want.sum(0) - flat).abs() <= 2.0 ** -22 * want.abs().sum(0)).all())  # the contract's sums, cut by workgroup
    worst = 0.0
    for order in ("torch", "device"):
        part = restate_fp32(state, batch, 0.5, order)[2]["part"]
        assert part.shape == want.shape == bound.shape == (X.blocks(B), X.OUT)
        worst = max(worst, _partial_share(part, want, bound))
    assert worst <= 1.0, worst
    least = float("inf")
    for defect in PARTIAL_DEFECTS:
        if defect == "tile_to_wrong_workgroup" and B <= 128:
            continue  # one workgroup: there is no wrong one
        part = restate_fp32(state, batch, 0.5, "device", defect)[2]["part"]
        share = _partial_share(part, want, bound)
        least = min(least, share)
        assert share > 1.0, (defect, share)
        if defect == "tile_to_wrong_workgroup":
            out = ((part.double() - want).abs() > bound).any(dim=1).nonzero().view(-1).tolist()
            assert out == [0, 1], out
    print("\nF%d_B%d per-partial bound: clean restatements use %.3g of it, the mildest defect %.3g x" % (F, B, worst, least))
