"""The joint training step (layer1 trained under the collect heads) restated twice, for the tests of
antsrl_jointtrain_step:

  fp32_train_step      the reference's arithmetic with the freeze of layer1 lifted and nothing else changed:
                       CollectAgent.train (agents/collect_agent.py:105-148) in torch fp32 with autograd on all six tensors,
                       then torch.optim.Adam's single-tensor update — what joint_train_ref.npz records;
  contract_train_step  the device contract of include/antsrl.h: layer1 on bfloat16-rounded x and w1 (products exact in fp32,
                       summed in float64 here), h and h' through the SAME live w1, everything behind it from the closed
                       forms  dq = 2 d / (3 B) at the taken action per head,
                       dh = dq_rot w2[a_rot] + dq_ph w3[a_ph] (two fp32 products, one fp32 add),
                       g_w1 = dh^T bf16(x), g_b1 = sum_b dh.

bf16_bounds bounds the contract against fp32 from bfloat16's unit roundoff; fp32_sum_bounds bounds a device against the
contract from the order of fp32 sums alone.  Both are dqn_ref.propagate_head per head (linear_train_ref.py's use of it)
and explore_train_ref.py's layer1 terms, with the one extra add of dh.

`state`: linear_train_ref's with Adam's moments for all six tensors: sd (the six tensors under CollectModel's names),
target_w3 / target_b3, m / v by name, step.  `batch` = (states [B, F], agent_states [B, 2], actions [B, 2], rewards [B],
new_states, new_agent_states, dones [B]), already gathered.  Both steps return (loss, grads by name)."""
from functools import partial

import numpy as np
import torch

import dqn_ref as D
import linear_train_cases as LC
import linear_train_ref as L
from dqn_ref import U_BF16, U_FP32, bf16, gamma, gather  # noqa: F401
from dqn_ref import as_batch as _t
from linear_train_ref import sync_target  # noqa: F401  (target := model: layer3 is all the two nets do not share)

NAMES = L.NAMES
W1, B1, W2, B2, W3, B3 = NAMES
adam = partial(D.adam, NAMES)                      # (state, grads, lr, betas, eps): Adam over all six tensors
worst_share = partial(D.worst_share, keys=NAMES)   # (got, want, bound)


def new_state(sd, target=None):
    """target: (w3, b3) of the target net's layer3, the model's by default."""
    sd = {k: torch.as_tensor(np.asarray(sd[k]), dtype=torch.float32).clone() for k in NAMES}
    tw3, tb3 = (sd[W3], sd[B3]) if target is None else target
    return dict(sd=sd, target_w3=torch.as_tensor(np.asarray(tw3), dtype=torch.float32).clone(),
                target_b3=torch.as_tensor(np.asarray(tb3), dtype=torch.float32).clone(),
                m={k: torch.zeros_like(sd[k]) for k in NAMES}, v={k: torch.zeros_like(sd[k]) for k in NAMES}, step=0)


def _clamped(batch):
    st, ast, act, rw, nst, nast, dn = _t(batch)
    return st, ast, act.clamp(0, 2), rw, nst, nast, dn  # (the clamp is the device contract's: the reference would raise)


def fp32_train_step(state, batch, discount=0.5, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, update=True):
    st, ast, act, rw, nst, nast, dn = _clamped(batch)
    p = {k: state["sd"][k].clone().requires_grad_(True) for k in NAMES}

    def net(x, a, w3, b3):
        out = torch.cat([x, a], dim=1) @ p[W1].T + p[B1]
        return out @ p[W2].T + p[B2], out @ w3.T + b3
    rows = torch.arange(len(rw))
    with torch.no_grad():
        fr, fp = net(nst, nast, state["target_w3"], state["target_b3"])  # the target net: the live layer1 and layer2
        tr, tp = net(st, ast, p[W3], p[B3])
        tr, tp = tr.clone(), tp.clone()
        tr[rows, act[:, 0]] = rw + discount * fr.max(dim=1).values * ~dn
        tp[rows, act[:, 1]] = rw + discount * fp.max(dim=1).values * ~dn
    qr, qp = net(st, ast, p[W3], p[B3])
    loss = torch.nn.functional.mse_loss(qr, tr) + torch.nn.functional.mse_loss(qp, tp)
    loss.backward()
    grads = {k: p[k].grad.detach().clone() for k in NAMES}
    if update:
        adam(state, grads, lr, betas, eps)
    return float(loss.detach()), grads


def contract_forward(state, batch, discount=0.5):
    """linear_train_ref.contract_forward (the forward is the frozen step's: one layer1 for h and h') on clamped actions,
    and xe = bf16(x ++ agent_state), the layer1 gradient's right operand."""
    b = _clamped(batch)
    f = L.contract_forward(state, b, discount)
    f["xe"] = bf16(torch.cat([b[0], b[1]], 1))
    return f


def contract_backward(state, f):
    """From contract_forward's f, in fp32: dq [B, 7] (dL/dq of both heads at the taken actions, then the row's loss term)
    and dh [B, 32] = dq_rot w2[a_rot] + dq_ph w3[a_ph]: two products and one add per element, each rounded on its own."""
    dr, dp, act = f["dr"], f["dp"], f["act"]
    B = len(dr)
    scale, inv = float(np.float32(2.0 / (3.0 * B))), float(np.float32(1.0 / (3.0 * B)))
    gr, gp = dr * scale, dp * scale
    rows = torch.arange(B)
    dq = torch.zeros((B, 7), dtype=torch.float32)
    dq[rows, act[:, 0]] = gr
    dq[rows, 3 + act[:, 1]] = gp
    dq[:, 6] = dr * dr * inv + dp * dp * inv
    sd = state["sd"]
    return dq, gr[:, None] * sd[W2][act[:, 0]] + gp[:, None] * sd[W3][act[:, 1]]


def contract_train_step(state, batch, discount=0.5, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, update=True):
    f = contract_forward(state, batch, discount)
    h = f["h"]
    dq, dh = contract_backward(state, f)
    loss = float(dq[:, 6].double().sum())
    gw = (dq[:, :6].double().T @ h.double()).to(torch.float32)
    gb = dq[:, :6].double().sum(0).to(torch.float32)
    grads = {W1: (dh.double().T @ f["xe"].double()).to(torch.float32), B1: dh.double().sum(0).to(torch.float32),
             W2: gw[:3].clone(), B2: gb[:3].clone(), W3: gw[3:].clone(), B3: gb[3:].clone()}
    if update:
        adam(state, grads, lr, betas, eps)
    return loss, grads


def _bounds(state, batch, discount, h, hn, eh, ehn, xe, exe, own, elem, rowsum, loss_elem, add):
    """A forward error bound carried to the loss and to every gradient.  h, hn: the hidden values of the rows and of their
    successors (both under the one live layer1), eh, ehn what they may be off by; xe [B, F + 2] the layer1 gradient's
    right operand and exe what IT may be off by (float64).  Each head is dqn_ref.propagate_head's (e_q, e_y, e_d, the
    loss, its weight and bias gradients); from the heads' d and e_d, layer1 as explore_train_ref._bounds has it, summed
    over the two heads, with `add` for the one addition that joins them:
        dh:    m[b][j]    = 2 / (3 B) (|d_rot| |w2[a_rot][j]| + |d_ph| |w3[a_ph][j]|)          the magnitude of its terms
               e_dh[b][j] = 2 / (3 B) sum_heads (e_d + elem (|d| + e_d)) |w[a][j]|  +  add (m + the sum in front)
        g_w1:  sum_b (e_dh (|xe| + e_xe) + m e_xe)  +  rowsum sum_b (m + e_dh) (|xe| + e_xe)
        g_b1:  the same with xe := 1, e_xe := 0.
    Key "dh" holds e_dh, key "loss" the two heads' loss bounds added."""
    st, ast, act, rw, nst, nast, dn = _clamped(batch)
    sd = state["sd"]
    live = (~dn).double()
    heads = ((sd[W2], sd[B2], sd[W2], sd[B2], act[:, 0]),                       # rotation: the target net shares layer2
             (sd[W3], sd[B3], state["target_w3"], state["target_b3"], act[:, 1]))
    c = 2.0 / (3 * len(rw))
    out = {"loss": 0.0}
    mag = edh = 0.0
    for i, head in enumerate(heads):
        loss, out[NAMES[2 + 2 * i]], out[NAMES[3 + 2 * i]], d, ed = D.propagate_head(
            *head, rw, live, discount, h, hn, eh, ehn, own, elem, rowsum, loss_elem)
        out["loss"] += loss
        wa = head[0].double()[head[4]].abs()                                     # [B, 32]
        mag = mag + c * d.abs()[:, None] * wa
        edh = edh + c * (ed + elem * (d.abs() + ed))[:, None] * wa
    edh = edh + add * (mag + edh)
    out[W1] = edh.T @ (xe.abs() + exe) + mag.T @ exe + rowsum * ((mag + edh).T @ (xe.abs() + exe))
    out[B1] = edh.sum(0) + rowsum * (mag + edh).sum(0)
    out["dh"] = edh  # [B, 32]: what dh itself may be off by
    return out


def bf16_bounds(state, batch, discount=0.5):
    """How far the contract may stand from fp32, from bfloat16's unit roundoff u = 2^-9 alone.  x and w1 are each rounded
    once in the forward, so a product is off by at most (2 u + u^2) |x w|: e_h = (2 u + u^2) (|x| |w1|^T), for h and h'
    alike (one layer1); the layer1 gradient's x is rounded once: e_xe = u |x|.  d, h taken from the fp32 forward; fp32
    summation adds 2^-24-sized terms on top, far below (fp32_sum_bounds)."""
    st, ast, act, rw, nst, nast, dn = _clamped(batch)
    sd = state["sd"]
    c = 2 * U_BF16 + U_BF16 ** 2
    x, xn = torch.cat([st, ast], 1).double(), torch.cat([nst, nast], 1).double()
    w1, b1 = sd[W1].double(), sd[B1].double()
    eh, ehn = c * (x.abs() @ w1.abs().T), c * (xn.abs() @ w1.abs().T)
    return _bounds(state, batch, discount, x @ w1.T + b1, xn @ w1.T + b1, eh, ehn, x, U_BF16 * x.abs(), 0.0, 0.0, 0.0, 0.0, 0.0)


def fp32_sum_bounds(state, batch, discount=0.5):
    """An a-priori bound on |device - contract_train_step| per tensor (elementwise, float64) and for the loss (key
    "loss"), from the order of fp32 sums alone; nothing is read from a device.  Operands are equal on both sides (the
    bfloat16 roundings are part of the contract), so all that differs is where sums round.  With u = 2^-24 and
    gamma(n) = n u / (1 - n u):
        layer1   e_h = gamma(F + 3) (|bf16 x| |bf16 w1|^T + |b1|)     for h and h', under the one live w1
        heads    that error through |W|, and gamma(34) on the head's own sum of 32 products and a bias
        y, d     4 u on the operands (discount * max, + reward, q - y, the restatement's own rounding)
        dh       each head's d error through w[a]; 4 u for the two roundings of d * scale * w[a][j] on either side;
                 2 u for the addition of the two products, one rounding on either side
        rows     gamma(B + 2) sum_b |term| for every gradient alike: B - 1 additions, the product, the restatement's
                 rounding (bf16 x is exact on both sides: e_xe = 0)
        loss     gamma(4) more per term."""
    h, hn, eh, ehn, xe = _sum_bound_hidden(state, batch)
    return _bounds(state, batch, discount, h, hn, eh, ehn, xe, torch.zeros_like(xe), gamma(34), 4 * U_FP32,
                   gamma(len(batch[3]) + 2), gamma(4), 2 * U_FP32)


def _sum_bound_hidden(state, batch):
    """Layer1 under fp32_sum_bounds: h, h', what they may be off by, and xe (float64)."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    F = st.shape[1]
    w1, b1 = bf16(state["sd"][W1]).double(), state["sd"][B1].double()

    def hidden(x, a):
        xa = bf16(torch.cat([x, a], 1)).double()
        return xa, xa @ w1.T + b1, gamma(F + 3) * (xa.abs() @ w1.abs().T + b1.abs())
    (xe, h, eh), (_, hn, ehn) = hidden(st, ast), hidden(nst, nast)
    return h, hn, eh, ehn, xe


# ---- the workspace (antsrl_jointtrain.hip): the forward stage's partials, then dh ---------------------------------------
OUT = L.OUT    # 199: the 198 head gradients in the flat block's order (w2, b2, w3, b3), then the loss
PART = L.PART  # 200 floats per workgroup


def blocks(B):
    """Workgroups of the forward stage (antsrl_jointtrain_blocks): four tiles of 32 rows each, one per wave, no looping."""
    return ((B + 31) // 32 + 3) // 4


def work_layout(B):
    """The workspace of a step on B rows: partials [blocks][PART] fp32 from byte 0, dh [B][32] fp32 at the next multiple
    of 256 bytes, nothing behind row B - 1."""
    dh = (blocks(B) * PART * 4 + 255) // 256 * 256
    return dict(blocks=blocks(B), dh_offset=dh, bytes=dh + B * 32 * 4)


def row_workgroup(B):
    """[B] int64: tile t = b // 32 belongs to workgroup t // 4 (wave t % 4)."""
    return torch.arange(B) // 128


row_terms = L.row_terms  # dq [B, 7] and h [B, 32] -> [B, OUT]: what each row adds to the forward stage's outputs
ordered_sum = L.ordered_sum


def device_order_sum(terms, B):
    """terms [B, n] fp32 -> ([n], [blocks, n]): the row sums in the order of k_jointtrain_fwd and the last workgroup of
    k_jointtrain_l1, and the workgroups' partials on the way (a wave's one tile row by row from zero, the workgroup's four
    waves, then the workgroups)."""
    nb = blocks(B)
    pad = torch.zeros((nb * 128, terms.shape[1]), dtype=torch.float32)
    pad[:B] = terms
    pad = pad.view(nb, 4, 32, -1)
    out = torch.zeros((nb, 4, terms.shape[1]), dtype=torch.float32)
    for r in range(32):
        out = out + pad[:, :, r]
    part = torch.zeros((nb, terms.shape[1]), dtype=torch.float32)
    for w in range(4):
        part = part + out[:, w]
    return ordered_sum(part), part


def expected_partials(state, batch, discount=0.5):
    """[blocks, OUT] float64: every workgroup's partial from contract_forward's h and d, the products and the sums over
    the workgroup's rows in float64."""
    f = contract_forward(state, batch, discount)
    B = len(f["dr"])
    dq, _ = contract_backward(state, f)
    return torch.zeros((blocks(B), OUT), dtype=torch.float64).index_add_(0, row_workgroup(B), row_terms(dq.double(), f["h"].double()))


def partial_bounds(state, batch, discount=0.5):
    """fp32_sum_bounds' heads and loss for one workgroup's partial at a time, [blocks, OUT] float64: the terms summed over
    that workgroup's rows only, with the batch's B in 2 / (3 B) and 1 / (3 B), and gamma(rows + 4 + 2) for the row sums,
    rows being the workgroup's (the rows, the wave adds, the product and the restatement's rounding)."""
    st, ast, act, rw, nst, nast, dn = _clamped(batch)
    sd = state["sd"]
    B = len(rw)
    h, hn, eh, ehn, _ = _sum_bound_hidden(state, batch)
    group = row_workgroup(B)
    rowsum = gamma(torch.bincount(group, minlength=blocks(B)).double() + 6)
    heads = ((sd[W2], sd[B2], sd[W2], sd[B2], act[:, 0]), (sd[W3], sd[B3], state["target_w3"], state["target_b3"], act[:, 1]))
    out = torch.zeros((blocks(B), OUT), dtype=torch.float64)
    for i, head in enumerate(heads):
        loss, gw, gb = D.propagate_head_grouped(*head, rw, (~dn).double(), discount, h, hn, eh, ehn, group, rowsum,
                                                own=gamma(34), elem=4 * U_FP32, loss_elem=gamma(4))[:3]
        out[:, 99 * i: 99 * i + 96], out[:, 99 * i + 96: 99 * i + 99] = gw.reshape(-1, 96), gb
        out[:, 198] += loss
    return out


# ---- the cases the test files share -------------------------------------------------------------------------------------
def make_case(F, B, seed, N=None, dones="some"):
    """A net (with a target layer3 that differs from the model's), a replay of N rows and B indices into it, on the CPU.
    The observations and agent states are linear_train_cases': half of the observations zero, the others signed, one in
    eight of them an exact bfloat16 tie, a tie of each kind in every row where F >= 3, a dense large last column; agent
    states a fifth of a bfloat16 spacing above a bfloat16 value, so that every one of them rounds.  Weights are
    nn.Linear's init, scaled up 3 x in both heads so that dh, and with it layer1's gradient, is not small against the
    heads'.  Rewards are normal with the scale of the rows' own q, the mean of both heads' |q| + 1: both heads' TD errors
    are then of the size of their q, neither small against the other.  With dones="some" the batch holds a live row whose two
    actions differ (its first) and, from two rows on, a done row (its last): what a defect needs to show.
    Returns (state, arrays, idx)."""
    g = torch.Generator().manual_seed(seed)
    N = N or max(3 * B // 2 + 7, 40)
    IN = F + 2
    u = lambda shape, b: (torch.rand(shape, generator=g) * 2 - 1) * b  # noqa: E731
    sd = {W1: u((32, IN), IN ** -0.5), B1: u((32,), IN ** -0.5), W2: u((3, 32), 3 * 32 ** -0.5), B2: u((3,), 32 ** -0.5),
          W3: u((3, 32), 3 * 32 ** -0.5), B3: u((3,), 32 ** -0.5)}
    state = new_state(sd, (u((3, 32), 3 * 32 ** -0.5), u((3,), 32 ** -0.5)))
    wide = LC._wide(F)
    big, as_exp = wide.get("big", 1.0), wide.get("as_exp", 10)
    st, nst = LC._observations(g, N, F, big), LC._observations(g, N, F, big)

    def agent_states():
        a = 2.0 ** (torch.rand((N, 2), generator=g, dtype=torch.float64) * as_exp)
        a = (a * (torch.randint(0, 2, (N, 2), generator=g).double() * 2 - 1)).float().to(torch.bfloat16).double()
        spacing = 2.0 ** (torch.floor(torch.log2(a.abs())) - 7)
        return (a + 0.2 * spacing).float()
    ast, nast = agent_states(), agent_states()
    act = torch.randint(0, 3, (N, 2), generator=g)
    dn = {"some": torch.rand((N,), generator=g) < 0.3, "all": torch.ones((N,), dtype=torch.bool),
          "none": torch.zeros((N,), dtype=torch.bool)}[dones]
    idx = torch.randint(0, N, (B,), generator=g)
    if dones == "some":  # the batch's first row is live and took two different actions; its last row (B >= 2) is done
        idx[0], idx[B - 1] = 0, min(1, B - 1)
        dn[0], dn[1] = False, True
        act[0] = torch.tensor([0, 2])
    hid = bf16(torch.cat([st, ast], 1)).double() @ bf16(sd[W1]).double().T + sd[B1].double()
    rows = torch.arange(N)
    qr = (hid @ sd[W2].double().T + sd[B2].double())[rows, act[:, 0]]
    qp = (hid @ sd[W3].double().T + sd[B3].double())[rows, act[:, 1]]
    rw = (torch.randn((N,), generator=g, dtype=torch.float64) * (0.5 * (qr.abs() + qp.abs()) + 1)).float()
    return state, (st, ast, act, rw, nst, nast, dn), idx


#: (F, B): the smallest shapes at which each seam of antsrl_jointtrain.hip exists — one row, a partial and a full 32-row
#: tile, more than one tile / wave / workgroup of the forward stage (31 / 32 / 33, 512 / 513), F below one k-step, F not a
#: multiple of 4, 8 or 16, a column slab that straddles states | agent_state | bias, 608 / 609 either side of 64 KiB of
#: LDS, the widest rows, the reference's 264 rows, and batches of many workgroups up to the limit of 65 536 rows
SHAPES = ((1, 1), (1, 33), (17, 31), (17, 32), (17, 33), (17, 513), (294, 264), (294, 512), (294, 513), (607, 33), (608, 33),
          (609, 33), (1022, 33), (1022, 264), (17, 4096), (17, 65536))
#: further cases at F = 17, B = 40: name -> (make_case keywords, discount)
VARIANTS = {"idx_null": ({}, 0.5), "idx_clamped": ({}, 0.5), "actions_clamped": ({}, 0.5), "dones_all": (dict(dones="all"), 0.5),
            "dones_none": (dict(dones="none"), 0.5), "discount_0": ({}, 0.0), "discount_0.99": ({}, 0.99),
            "nan_ring": ({}, 0.5)}


def shape_case(F, B):
    """make_case at a SHAPES shape (a ring of 3000 rows under the large batches)."""
    return make_case(F, B, 100 * F + B, N=3000 if B > 4096 else None)


def lds_bytes(F):
    """Dynamic LDS of the forward stage at width F (jt_lds, antsrl_jointtrain.hip): k_lintrain's with four waves."""
    return LC.lds_bytes(F, 4)


def make_variant(name):
    """(state, arrays, idx or None, discount, B) of a VARIANTS case; `arrays` is what the device gets (out-of-range
    values, NaN rows and all)."""
    kw, discount = VARIANTS[name]
    F, B = 17, 40
    state, arrays, idx = make_case(F, B, 1000 + sorted(VARIANTS).index(name), **kw)
    st, ast, act, rw, nst, nast, dn = arrays
    N = st.shape[0]
    if name == "idx_null":  # without idx the minibatch is rows 0 .. B - 1 of the arrays, all of them: B rows are handed over
        arrays = tuple(t[:B].clone() for t in arrays)
        st, ast, act, rw, nst, nast, dn = arrays
        N, idx = B, None
    elif name == "idx_clamped":
        idx[::5] = torch.tensor([-1, N, -(1 << 40), 1 << 40, N + 3, -7, N, -1])
    elif name == "actions_clamped":
        act[::3, 0] = torch.tensor([-1, 3, 7, -(1 << 33), 1 << 33] * 20)[: len(act[::3])]
        act[1::3, 1] = torch.tensor([5, -2, 1 << 33, 3, -(1 << 33)] * 20)[: len(act[1::3])]
    elif name == "nan_ring":
        keep = torch.zeros((N,), dtype=torch.bool)
        keep[idx] = True
        for t in (st, ast, rw, nst, nast):
            t[~keep] = float("nan")
    return state, arrays, idx, discount, B


def gather_clamped(arrays, idx, B):
    """The minibatch rows as the device takes them: row idx[b] clamped to [0, N), or row b without idx."""
    N = arrays[0].shape[0]
    rows = torch.arange(B) if idx is None else idx.clamp(0, N - 1)
    return gather(arrays, rows)
