"""The linear agent's training step restated twice, for the tests of antsrl_lintrain_step:

  fp32_train_step      the reference's arithmetic: CollectAgent.train (agents/collect_agent.py:105-148) in torch fp32 with
                       autograd, then torch.optim.Adam's single-tensor update — what linear_train_ref.npz records;
  contract_train_step  the device contract of include/antsrl.h: layer1 on bfloat16-rounded x and w1 (the products are
                       exact in fp32; they are summed in float64 here, the MFMA sums them in fp32), everything behind
                       it in fp32 from the closed form  dL/dq = 2 (q - y) / (3 B) at the taken action.

bf16_bounds bounds contract against fp32 from bfloat16's unit roundoff; fp32_sum_bounds bounds a device against the contract
from the order of fp32 sums alone (the bound of the shapes beyond F = 294: linear_train_cases.py).

Both restatements take and update a `state` dict: sd (the six tensors under CollectModel's names), target_w3 / target_b3, m / v (Adam's
moments of the four trained tensors, by name), step.  `batch` = (states [B, F], agent_states [B, 2], actions [B, 2],
rewards [B], new_states, new_agent_states, dones [B]), already gathered.  Both return (loss, grads by name)."""
from functools import partial

import numpy as np
import torch

import dqn_ref as D
from dqn_ref import U_BF16, U_FP32, bf16, gamma  # noqa: F401
from dqn_ref import as_batch as _t

NAMES = ("explore_model.layer1.weight", "explore_model.layer1.bias", "explore_model.layer2.weight",
         "explore_model.layer2.bias", "layer3.weight", "layer3.bias")
TRAINED = NAMES[2:]
adam = partial(D.adam, TRAINED)                      # (state, grads, lr, betas, eps): Adam over the four trained tensors
worst_share = partial(D.worst_share, keys=TRAINED)   # (got, want, bound)


def new_state(sd):
    sd = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32).clone() for k, v in sd.items()}
    return dict(sd=sd, target_w3=sd["layer3.weight"].clone(), target_b3=sd["layer3.bias"].clone(),
                m={k: torch.zeros_like(sd[k]) for k in TRAINED}, v={k: torch.zeros_like(sd[k]) for k in TRAINED}, step=0)


def sync_target(state):
    state["target_w3"], state["target_b3"] = state["sd"]["layer3.weight"].clone(), state["sd"]["layer3.bias"].clone()


def fp32_train_step(state, batch, discount=0.5, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, update=True):
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd = state["sd"]
    p = {k: sd[k].clone().requires_grad_(k in TRAINED) for k in NAMES}

    def net(x, a, w3, b3):
        out = torch.cat([x, a], dim=1) @ p[NAMES[0]].T + p[NAMES[1]]
        return out @ p[NAMES[2]].T + p[NAMES[3]], out @ w3.T + b3
    rows = torch.arange(len(rw))
    with torch.no_grad():
        fr, fp = net(nst, nast, state["target_w3"], state["target_b3"])  # the target net: shared layer1 and layer2
        tr, tp = net(st, ast, p[NAMES[4]], p[NAMES[5]])
        tr, tp = tr.clone(), tp.clone()
        tr[rows, act[:, 0]] = rw + discount * fr.max(dim=1).values * ~dn
        tp[rows, act[:, 1]] = rw + discount * fp.max(dim=1).values * ~dn
    qr, qp = net(st, ast, p[NAMES[4]], p[NAMES[5]])
    loss = torch.nn.functional.mse_loss(qr, tr) + torch.nn.functional.mse_loss(qp, tp)
    loss.backward()
    grads = {k: p[k].grad.detach().clone() for k in TRAINED}
    if update:
        adam(state, grads, lr, betas, eps)
    return float(loss.detach()), grads


def contract_hidden(sd, x, a):
    """layer1 as the device computes it: [B, 32] fp32."""
    w1, b1 = sd[NAMES[0]], sd[NAMES[1]]
    F = x.shape[1]
    acc = (bf16(x).double() @ bf16(w1[:, :F]).double().T).to(torch.float32)
    wa, aa = bf16(w1[:, F:]), bf16(a)
    return acc + (aa[:, 0:1] * wa[:, 0] + aa[:, 1:2] * wa[:, 1]) + b1


def contract_forward(state, batch, discount=0.5):
    """h, the d = q - y of both heads, and what they are made of (all fp32)."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd = state["sd"]
    h, hn = contract_hidden(sd, st, ast), contract_hidden(sd, nst, nast)
    lin = lambda v, w, b: (v.double() @ w.double().T).to(torch.float32) + b  # noqa: E731
    qr, qp = lin(h, sd[NAMES[2]], sd[NAMES[3]]), lin(h, sd[NAMES[4]], sd[NAMES[5]])
    nr, npq = lin(hn, sd[NAMES[2]], sd[NAMES[3]]), lin(hn, state["target_w3"], state["target_b3"])
    live = (~dn).to(torch.float32)
    rows = torch.arange(len(rw))
    yr = rw + discount * nr.max(dim=1).values * live
    yp = rw + discount * npq.max(dim=1).values * live
    return dict(h=h, hn=hn, qr=qr, qp=qp, nr=nr, np=npq, dr=qr[rows, act[:, 0]] - yr, dp=qp[rows, act[:, 1]] - yp, act=act)


def contract_train_step(state, batch, discount=0.5, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, update=True):
    f = contract_forward(state, batch, discount)
    B = len(f["dr"])
    h, act = f["h"], f["act"]
    scale, inv = np.float32(2.0 / (3.0 * B)), np.float32(1.0 / (3.0 * B))
    dq = torch.zeros((B, 6), dtype=torch.float32)
    rows = torch.arange(B)
    dq[rows, act[:, 0]] = f["dr"] * float(scale)
    dq[rows, 3 + act[:, 1]] = f["dp"] * float(scale)
    loss = float((f["dr"] * f["dr"] * float(inv) + f["dp"] * f["dp"] * float(inv)).double().sum())
    gw = (dq.double().T @ h.double()).to(torch.float32)
    gb = dq.double().sum(dim=0).to(torch.float32)
    grads = {NAMES[2]: gw[:3].clone(), NAMES[3]: gb[:3].clone(), NAMES[4]: gw[3:].clone(), NAMES[5]: gb[3:].clone()}
    if update:
        adam(state, grads, lr, betas, eps)
    return loss, grads


def _heads(state, act):
    """Per head what D.propagate_head takes first: (W, b, the target's W, b, the action taken)."""
    sd = state["sd"]
    return ((sd[NAMES[2]], sd[NAMES[3]], sd[NAMES[2]], sd[NAMES[3]], act[:, 0]),  # rotation: the target net shares layer2
            (sd[NAMES[4]], sd[NAMES[5]], state["target_w3"], state["target_b3"], act[:, 1]))


def bf16_bounds(state, batch, discount=0.5):
    """How far the contract may stand from fp32, from bfloat16's unit roundoff u = 2^-9 alone.  x and w1 are each
    rounded once, so a product is off by at most (2 u + u^2) |x w|:
        e_h  = (2 u + u^2) (|x| |w1|^T)                         per hidden value           [B, 32]
    carried through the heads, the TD target, the loss and the gradient sums by dqn_ref.propagate_head, with d, h taken from the
    fp32 forward.  fp32 summation adds a slack of the order 2^-24 * (terms) on top, far below (fp32_sum_bounds)."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd = state["sd"]
    c = 2 * U_BF16 + U_BF16 ** 2
    w1 = sd[NAMES[0]].double().abs()
    eh = c * (torch.cat([st, ast], 1).double().abs() @ w1.T)
    ehn = c * (torch.cat([nst, nast], 1).double().abs() @ w1.T)
    hfun = lambda x, a: torch.cat([x, a], 1).double() @ sd[NAMES[0]].double().T + sd[NAMES[1]].double()  # noqa: E731
    h, hn = hfun(st, ast), hfun(nst, nast)
    live = (~dn).double()
    out = {}
    for i, head in enumerate(_heads(state, act)):
        out[("loss", i)], out[NAMES[2 + 2 * i]], out[NAMES[3 + 2 * i]] = D.propagate_head(*head, rw, live, discount, h, hn, eh, ehn)[:3]
    out["h"] = eh
    return out


def fp32_sum_bounds(state, batch, discount=0.5):
    """An a-priori bound on |device - contract_train_step| per trained tensor (elementwise, float64) and for the loss
    (key "loss"), from the order of fp32 sums alone; nothing is read from a device.  Operands are equal on both sides (the
    bfloat16 roundings are part of the contract, and their products are exact in fp32), so all that differs is where the
    sums round: contract_train_step sums in float64 and rounds once, a device sums in fp32 in an order of its own.  With
    u = 2^-24 and gamma(n) = n u / (1 - n u), whatever the order:
        layer1   e_h = gamma(F + 3) (|bf16 x| |bf16 w1|^T + |b1|)     F + 2 products and the bias: at most F + 3 roundings
        heads    that error through |W|, and gamma(34) on the head's own sum of 32 products and a bias
        y, d     a rounding each for discount * max, + reward, q - y, and the restatement's own: 4 u on the operands
        rows     gamma(B + 2) sum_b |term|: B - 1 additions, the product, the 2 / (3 B) scaling and the restatement's rounding
        loss     gamma(4) more per term: d * d, * 1 / (3 B), twice, and the sum of the two heads
    carried to d, the loss and the gradients by dqn_ref.propagate_head, as bf16_bounds carries 2 u + u^2."""
    B = len(batch[3])
    out = {"loss": 0.0}
    for i, head in enumerate(_sum_bound_heads(state, batch, discount)):
        loss, out[NAMES[2 + 2 * i]], out[NAMES[3 + 2 * i]] = D.propagate_head(
            *head, own=gamma(34), elem=4 * U_FP32, rowsum=gamma(B + 2), loss_elem=gamma(4))[:3]
        out["loss"] += loss
    return out


def _sum_bound_heads(state, batch, discount):
    """Per head, propagate_head's arguments up to e_h' under fp32_sum_bounds: layer1 and what it may be off by."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd = state["sd"]
    F = st.shape[1]
    w1, b1 = bf16(sd[NAMES[0]]).double(), sd[NAMES[1]].double()

    def hidden(x, a):
        xa = bf16(torch.cat([x, a], 1)).double()
        return xa @ w1.T + b1, gamma(F + 3) * (xa.abs() @ w1.abs().T + b1.abs())
    (h, eh), (hn, ehn) = hidden(st, ast), hidden(nst, nast)
    return [head + (rw, (~dn).double(), discount, h, hn, eh, ehn) for head in _heads(state, act)]


# ---- the workspace of the gradient stage (antsrl_lintrain.hip): one row of partial sums per workgroup ----------------------
OUT = 199   # what a workgroup sums over its rows: the 198 gradients in the flat block's order (w2 [3][32] at 0, b2 at 96,
#             w3 [3][32] at 99, b3 at 195), then the loss term
PART = 200  # floats per workgroup in the workspace: OUT and one of padding


def blocks(B):
    """Workgroups of the gradient stage (antsrl_lintrain_blocks): one up to 16 tiles of 32 rows, which then finishes the
    step itself and leaves the workspace alone; else one per 4 tiles, at most 1024 (whose waves then loop)."""
    ntiles = (B + 31) // 32
    return 1 if ntiles <= 16 else min((ntiles + 3) // 4, 1024)


def work_layout(B):
    """The workspace of a step on B rows: partials [blocks][PART] fp32 from byte 0, nothing behind them."""
    return dict(blocks=blocks(B), bytes=blocks(B) * PART * 4)


def row_workgroup(B):
    """[B] int64: the workgroup whose partial row b goes into.  Tile t = b // 32 belongs to wave t % (4 blocks) of the
    grid, which is wave (t % (4 blocks)) % 4 of workgroup (t % (4 blocks)) // 4."""
    return (torch.arange(B) // 32) % (4 * blocks(B)) // 4


def device_order_sum(terms, B):
    """terms [B, n] fp32 -> ([n], [blocks, n]): the row sums in the order of k_lintrain and k_lintrain_finish, and the
    workgroups' partials on the way (a wave's tiles row by row, the workgroup's four waves, then the workgroups)."""
    ntiles, nb = (B + 31) // 32, blocks(B)
    waves = nb * 4
    rounds = (ntiles + waves - 1) // waves
    pad = torch.zeros((rounds * waves * 32, terms.shape[1]), dtype=torch.float32)
    pad[:B] = terms
    pad = pad.view(rounds, waves, 32, -1)  # tile t = round * waves + (block * 4 + wave in block)
    out = torch.zeros((waves, terms.shape[1]), dtype=torch.float32)
    for rd in range(rounds):
        for r in range(32):
            out = out + pad[rd, :, r]
    out = out.view(nb, 4, -1)
    part = torch.zeros((nb, terms.shape[1]), dtype=torch.float32)
    for w in range(4):
        part = part + out[:, w]
    return ordered_sum(part), part


def ordered_sum(part):
    """[blocks, n] fp32 -> [n]: the finish, a sequential fp32 sum from 0.0 in workgroup order."""
    s = torch.zeros((part.shape[1],), dtype=torch.float32)
    for b in range(part.shape[0]):
        s = s + part[b]
    return s


def row_terms(dq, h):
    """dq [B, 7] (the six dL/dq and the row's loss term) and h [B, 32] -> [B, OUT]: what each row adds to the outputs."""
    B = len(dq)
    h1 = torch.cat([h, torch.ones((B, 1), dtype=h.dtype)], 1)
    return torch.cat([(dq[:, :3, None] * h1[:, None, :32]).reshape(B, 96), dq[:, :3],
                      (dq[:, 3:6, None] * h1[:, None, :32]).reshape(B, 96), dq[:, 3:7]], 1)


def expected_partials(state, batch, discount=0.5):
    """[blocks, OUT] float64: every workgroup's partial from contract_forward's h and d, the products and the sums over
    the workgroup's rows in float64."""
    f = contract_forward(state, batch, discount)
    B = len(f["dr"])
    scale, inv = float(np.float32(2.0 / (3.0 * B))), float(np.float32(1.0 / (3.0 * B)))
    rows = torch.arange(B)
    dq = torch.zeros((B, 7), dtype=torch.float32)
    dq[rows, f["act"][:, 0]] = f["dr"] * scale
    dq[rows, 3 + f["act"][:, 1]] = f["dp"] * scale
    dq[:, 6] = f["dr"] * f["dr"] * inv + f["dp"] * f["dp"] * inv
    return torch.zeros((blocks(B), OUT), dtype=torch.float64).index_add_(0, row_workgroup(B), row_terms(dq.double(), f["h"].double()))


def partial_bounds(state, batch, discount=0.5):
    """fp32_sum_bounds for one workgroup's partial at a time, [blocks, OUT] float64: its terms summed over that
    workgroup's rows only, with the batch's B in 2 / (3 B) and 1 / (3 B), and gamma(rows + 4 + 2) for the row sums, rows
    being the workgroup's: a term passes through at most that many roundings on its way into the partial (the rows of
    its wave, the wave adds, the product) and the restatement adds its own."""
    B = len(batch[3])
    group = row_workgroup(B)
    rowsum = gamma(torch.bincount(group, minlength=blocks(B)).double() + 6)
    out = torch.zeros((blocks(B), OUT), dtype=torch.float64)
    for i, head in enumerate(_sum_bound_heads(state, batch, discount)):
        loss, gw, gb = D.propagate_head_grouped(*head, group, rowsum, own=gamma(34), elem=4 * U_FP32, loss_elem=gamma(4))[:3]
        out[:, 99 * i: 99 * i + 96], out[:, 99 * i + 96: 99 * i + 99] = gw.reshape(-1, 96), gb
        out[:, 198] += loss
    return out


def acting_gap_safe(w, x, head, nsig=4.0):
    """Which rows' fp32 decision of one head (0 rotation, 1 pheromone) the bfloat16 acting kernel must reproduce.

    The acting kernel rounds x and w1 (layer1's operands) and then h and the head's weights (its second MFMA) to bfloat16.
    Each rounding is a relative error in [-u, u], u = 2^-9, taken as independent and uniform (variance u^2 / 3), so a
    product of two rounded operands has relative variance 2 u^2 / 3:
        var h[j]   = (2 u^2 / 3) sum_k (x_k w1[j][k])^2
        var (q_a - q_b) = sum_j (W_a[j] - W_b[j])^2 var h[j]               (both heads read the same h: its error is shared)
                        + (2 u^2 / 3) sum_j (h[j]^2 + var h[j]) (W_a[j]^2 + W_b[j]^2)      (the head's own roundings)
    with a, b the fp32 top two.  A row is safe when the fp32 gap exceeds nsig = 4 standard deviations of that (a sum of
    some 300 independent terms: a 4-sigma excursion has probability below 1e-4).  fp32 accumulation adds 2^-24-sized
    terms, far below.  w: the six tensors by name (float64), x: [M, F + 2] float64.  Returns (safe [M] bool, argmax [M])."""
    u = U_BF16
    W1 = w[NAMES[0]]
    h = x @ W1.T + w[NAMES[1]]
    vh = (2 * u * u / 3) * ((x * x) @ (W1 * W1).T)
    W, b = w[NAMES[2 + 2 * head]], w[NAMES[3 + 2 * head]]
    q = h @ W.T + b
    top = q.topk(2, dim=1)
    Wa, Wb = W[top.indices[:, 0]], W[top.indices[:, 1]]
    dW = Wa - Wb
    vg = (vh * dW * dW).sum(1) + (2 * u * u / 3) * ((h * h + vh) * (Wa * Wa + Wb * Wb)).sum(1)
    return (top.values[:, 0] - top.values[:, 1]) > nsig * vg.sqrt(), top.indices[:, 0]
