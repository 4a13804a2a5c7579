"""linear_train_ref.fp32_sum_bounds is safe and sharp at every shape the device is tested at (linear_train_cases.CASES).

Safe: two fp32 restatements of the contract, which differ from contract_train_step only in where sums round, lie inside
the bound.  Layer1 is summed input by input in fp32 in one and in 16-input chunks (an exact chunk sum, one rounding: the
MFMA's k-step) in the other; both sum the rows in fp32 in the device's order: a wave's tiles row by row, the workgroup's
four waves, then the workgroups (linear_train_ref.device_order_sum).

Sharp: seven defective restatements, each one wrong thing a kernel could do, leave the bound on at least one gradient
element or on the loss.  The condition, which holds for every case and is not relaxed for any: a defect that changes
the function on the case's inputs must be outside the bound.  A case whose inputs hide a defect gets other inputs, never
another bound (linear_train_cases: a dense last column, ties in every row, large agent states at wide rows; below: the
cases that fix dones or discount take the mixed dones and the discount 0.5 for this half, and a ring of one row, which
cannot hold both kinds of dones, takes each in turn).  One defect is out of the bound's reach on some shapes by arithmetic
alone, whatever the inputs: 2 / (3 * 32 * ntiles) for 2 / (3 B) scales every sum by B / (32 ntiles).  Where 32 divides B
that IS the same number, and the test asserts equal bits.  Where 1 - B / (32 ntiles) < gamma(B + 2) (B = 131 233: 2.4e-4
against 7.8e-3) the change is at most that share of sum |term| and so below the bound's row-sum part on every element; the
test asserts that it moves the result and records that the bound cannot see it: at that size equal bits between
grad + apply and step, and the device's own measured error, are what guard the scale.  No shape is skipped.

The same two halves hold per workgroup (linear_train_cases.WORKSPACE, the shapes at which test_gpu_dqn_train_workspace.py
reads the workspace back): the restatements' partials lie inside linear_train_ref.partial_bounds of expected_partials, and
every defect, tile_to_wrong_workgroup among them, leaves it on at least one partial.  There the tile-count scale is within
reach at B = 131 233 too: a workgroup sums 256 rows at most, and gamma(262) is 1.6e-5."""
import numpy as np
import pytest
import torch

import linear_train_cases as K
import linear_train_ref as L

DEFECTS = ("drop_last_column", "agent_state_not_bf16", "model_l3_as_target", "dones_ignored", "last_row_left_out",
           "scale_by_tiles", "bf16_truncated")


def _bf16_trunc(x):
    return (torch.as_tensor(x, dtype=torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32)


def _layer1(xb, wb, chunked):
    """[B, F] x [32, F] -> [B, 32] in fp32: products of bfloat16 values are exact, the additions round."""
    B, F = xb.shape
    acc = torch.zeros((B, 32), dtype=torch.float32)
    if chunked:
        for k in range(0, F, 16):
            acc = acc + (xb[:, k:k + 16].double() @ wb[:, k:k + 16].double().T).float()
    else:
        for k in range(F):
            acc = acc + xb[:, k:k + 1] * wb[:, k]
    return acc


def restated(state, batch, discount, chunked=False, defect=None):
    """The contract in fp32 throughout (loss float, grads by name, the workgroups' partials), with one defect or none."""
    st, ast, act, rw, nst, nast, dn = L._t(batch)
    sd = state["sd"]
    B, F = st.shape
    rnd = _bf16_trunc if defect == "bf16_truncated" else L.bf16
    arnd = (lambda x: x) if defect == "agent_state_not_bf16" else rnd
    w1, b1 = sd[L.NAMES[0]], sd[L.NAMES[1]]
    wb, wa = rnd(w1[:, :F]), arnd(w1[:, F:])
    if defect == "drop_last_column":
        st, nst = st.clone(), nst.clone()
        st[:, F - 1] = 0.0
        nst[:, F - 1] = 0.0

    def hidden(x, a):
        a = arnd(a)
        return _layer1(rnd(x), wb, chunked) + (a[:, 0:1] * wa[:, 0] + a[:, 1:2] * wa[:, 1]) + b1
    h, hn = hidden(st, ast), hidden(nst, nast)
    lin = lambda v, w, b: v @ w.T + b  # noqa: E731
    tw3, tb3 = (sd[L.NAMES[4]], sd[L.NAMES[5]]) if defect == "model_l3_as_target" else (state["target_w3"], state["target_b3"])
    qr, qp = lin(h, sd[L.NAMES[2]], sd[L.NAMES[3]]), lin(h, sd[L.NAMES[4]], sd[L.NAMES[5]])
    nr, npq = lin(hn, sd[L.NAMES[2]], sd[L.NAMES[3]]), lin(hn, tw3, tb3)
    live = torch.ones((B,)) if defect == "dones_ignored" else (~dn).float()
    rows = torch.arange(B)
    dr = qr[rows, act[:, 0]] - (rw + discount * nr.max(dim=1).values * live)
    dp = qp[rows, act[:, 1]] - (rw + discount * npq.max(dim=1).values * live)
    n = 32 * ((B + 31) // 32) if defect == "scale_by_tiles" else B
    scale, inv = float(np.float32(2.0 / (3.0 * n))), float(np.float32(1.0 / (3.0 * n)))
    dq = torch.zeros((B, 7), dtype=torch.float32)
    dq[rows, act[:, 0]] = dr * scale
    dq[rows, 3 + act[:, 1]] = dp * scale
    dq[:, 6] = dr * dr * inv + dp * dp * inv
    if defect == "last_row_left_out":
        dq[B - 1] = 0.0
    terms = L.row_terms(dq, h)  # the 198 gradients, the loss
    if defect == "tile_to_wrong_workgroup":  # tiles 0 and 4 change places: the first tiles of workgroups 0 and 1
        terms = torch.cat([terms[128:160], terms[32:128], terms[0:32], terms[160:]])
    s, part = L.device_order_sum(terms, B)
    grads = {L.NAMES[2]: s[0:96].view(3, 32), L.NAMES[3]: s[96:99], L.NAMES[4]: s[99:195].view(3, 32), L.NAMES[5]: s[195:198]}
    return float(s[198]), grads, part


def _state(inp):
    s = L.new_state(inp["sd"])
    s["target_w3"], s["target_b3"] = inp["target"]
    return s


def _worst(loss, grads, loss_ref, g_ref, bound):
    """The largest |error| / bound over the loss and every gradient element (0 / 0 = 0; error over a zero bound = inf)."""
    f64 = lambda v: torch.as_tensor(v, dtype=torch.float64)  # noqa: E731
    return L.worst_share({**grads, "loss": f64(loss)}, {**g_ref, "loss": f64(loss_ref)}, bound, keys=L.TRAINED + ("loss",))


def test_the_lds_crossing_has_a_width_on_each_side():
    assert K.lds_bytes(608) <= 65536 < K.lds_bytes(609) and {607, 608, 609} <= set(K.WIDTHS)
    assert K.lds_bytes(1022) > 90000


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_fp32_restatements_are_inside_the_bound(case):
    inp = K.inputs(case)
    state, batch = _state(inp), K.gathered(inp, case["B"])
    loss_ref, g_ref = L.contract_train_step(state, batch, case["discount"], update=False)
    bound = L.fp32_sum_bounds(state, batch, case["discount"])
    for chunked in (False, True):
        loss, grads, _ = restated(state, batch, case["discount"], chunked)
        w = _worst(loss, grads, loss_ref, g_ref, bound)
        print("%s, layer1 %s: worst error / bound %.3g" % (case["name"], "in 16-input chunks" if chunked else "sequential", w))
        assert w <= 1.0


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_every_defect_leaves_the_bound(case):
    B = case["B"]
    discount = case["discount"] if case["name"] == "discount-0.99" else 0.5
    for defect in DEFECTS:
        # inputs under which the defect changes the function: mixed dones; a ring of one row is done for dones_ignored
        # (else the defect is the identity) and not done for the others (else the target net is never read)
        dones = ("all" if defect == "dones_ignored" else "none") if case["N"] == 1 else "mixed"
        inp = K.inputs(case, dones=dones, discount=discount)
        state, batch = _state(inp), K.gathered(inp, B)
        loss_ref, g_ref = L.contract_train_step(state, batch, discount, update=False)
        bound = L.fp32_sum_bounds(state, batch, discount)
        loss, grads, _ = restated(state, batch, discount, defect=defect)
        if defect == "scale_by_tiles" and B % 32 == 0:  # the same number: 32 * ntiles == B
            good_loss, good, _ = restated(state, batch, discount)
            assert loss == good_loss and all(torch.equal(grads[k], good[k]) for k in L.TRAINED)
            continue
        w = _worst(loss, grads, loss_ref, g_ref, bound)
        print("%s, %s: worst error / bound %.3g" % (case["name"], defect, w))
        if defect == "scale_by_tiles" and 1.0 - B / (32.0 * ((B + 31) // 32)) < L.gamma(B + 2):
            assert w > 0.0  # a change, but one no summation-order bound can tell from a permitted order
            continue
        assert w > 1.0, (case["name"], defect, w)


# ---- the workgroups' partials: what test_gpu_dqn_train_workspace.py reads back from the workspace ----------------------
def _partial_share(part, want, bound):
    """The largest |partial - expected| / bound over [workgroup][output] (0 / 0 = 0; an error over a zero bound = inf)."""
    err = (part.double() - want).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


@pytest.mark.parametrize("case", K.WORKSPACE, ids=K.WORKSPACE_IDS)
def test_the_workspace_layout_is_the_librarys(case):
    import ctypes as C
    from antsrl_amd import _lib
    from antsrl_amd import build as buildmod
    buildmod.build_hip()
    ws, launches = C.c_size_t(), C.c_int32()
    assert _lib.load().antsrl_lintrain_sizes(case["F"], case["B"], None, C.byref(ws), C.byref(launches)) == 0
    W = L.work_layout(case["B"])
    assert ws.value == W["bytes"] == W["blocks"] * L.PART * 4 and launches.value == 2 and W["blocks"] > 1
    group = L.row_workgroup(case["B"])
    assert int(group.max()) == min(W["blocks"], (case["B"] + 127) // 128) - 1 and int(torch.bincount(group).max()) <= 128 * -(-case["B"] // (128 * W["blocks"]))


@pytest.mark.parametrize("case", K.WORKSPACE, ids=K.WORKSPACE_IDS)
def test_fp32_partials_are_inside_the_per_partial_bound(case):
    inp = K.inputs(case)
    state, batch = _state(inp), K.gathered(inp, case["B"])
    want, bound = L.expected_partials(state, batch, case["discount"]), L.partial_bounds(state, batch, case["discount"])
    loss_ref, g_ref = L.contract_train_step(state, batch, case["discount"], update=False)
    total = want.sum(0)  # the partials are the contract's sums, cut by workgroup
    flat = torch.cat([g_ref[k].reshape(-1).double() for k in L.TRAINED] + [torch.tensor([loss_ref], dtype=torch.float64)])
    assert bool(((total - flat).abs() <= 2.0 ** -22 * want.abs().sum(0)).all())
    for chunked in (False, True):
        part = restated(state, batch, case["discount"], chunked)[2]
        assert part.shape == want.shape == bound.shape == (L.blocks(case["B"]), L.OUT)
        w = _partial_share(part, want, bound)
        print("%s, layer1 %s: worst partial error / bound %.3g" % (case["name"], "in 16-input chunks" if chunked else "sequential", w))
        assert w <= 1.0


@pytest.mark.parametrize("case", [c for c in K.WORKSPACE if c["dones"] == "mixed"], ids=lambda c: c["name"])
def test_every_defect_leaves_the_per_partial_bound(case):
    """The condition of test_every_defect_leaves_the_bound, on the partials: a defect that changes a partial leaves that
    partial's bound.  tile_to_wrong_workgroup changes no total beyond its rounding, and two partials entirely."""
    B = case["B"]
    inp = K.inputs(case, dones="mixed", discount=0.5)
    state, batch = _state(inp), K.gathered(inp, B)
    want, bound = L.expected_partials(state, batch, 0.5), L.partial_bounds(state, batch, 0.5)
    good = restated(state, batch, 0.5, chunked=True)[2]
    for defect in DEFECTS + ("tile_to_wrong_workgroup",):
        part = restated(state, batch, 0.5, chunked=True, defect=defect)[2]
        if defect == "scale_by_tiles" and B % 32 == 0:  # the same number: 32 * ntiles == B
            assert torch.equal(part, good)
            continue
        w = _partial_share(part, want, bound)
        print("%s, %s: worst partial error / bound %.3g" % (case["name"], defect, w))
        assert w > 1.0, (case["name"], defect, w)
        if defect == "tile_to_wrong_workgroup":
            out = ((part.double() - want).abs() > bound).any(dim=1).nonzero().view(-1).tolist()
            assert out == [0, 1], out
