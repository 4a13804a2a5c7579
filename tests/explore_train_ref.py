"""The explore agent's training step restated twice, for the tests of antsrl_exptrain_step:

  fp32_train_step      the reference's arithmetic as it was meant: ExploreModel (agents/explore_agent_pytorch.py:24-45) with
                       the concat of CollectModel.forward (agents/collect_agent.py:48), ExploreAgentPytorch.train (:90-133)
                       in torch fp32 with autograd on the CPU, then torch.optim.Adam's single-tensor update.  The class
                       cannot run as written, so this is a restatement and not a recorded run;
  contract_train_step  the device contract of include/antsrl.h: layer1 on bfloat16-rounded x and w1 (products exact in fp32,
                       summed in float64 here), everything behind it from the closed forms
                       dq = 2 d / (3 B) at the taken action, dh = dq w2[a], g_w1 = dh^T bf16(x), g_b1 = sum_b dh.

bf16_bounds bounds the contract against fp32 from bfloat16's unit roundoff; fp32_sum_bounds bounds a device against the
contract from the order of fp32 sums alone: linear_train_ref.py's method carried through one more layer.

`state`: sd (the four tensors under ExploreModel's names), target (the same four), m / v (Adam's moments by name), step.
`batch` = (states [B, F], agent_states [B, 2], actions [B, 2], rewards [B], new_states, new_agent_states, dones [B]),
already gathered.  Both steps return (loss, grads by name)."""
from functools import partial

import numpy as np
import torch

import dqn_ref as D
from dqn_ref import U_BF16, U_FP32, bf16, gamma, gather  # noqa: F401
from dqn_ref import as_batch as _t

NAMES = ("layer1.weight", "layer1.bias", "layer2.weight", "layer2.bias")
W1, B1, W2, B2 = NAMES
adam = partial(D.adam, NAMES)                      # (state, grads, lr, betas, eps): Adam over all four tensors
worst_share = partial(D.worst_share, keys=NAMES)   # (got, want, bound, keys=NAMES)


def new_state(sd, target=None):
    strip = lambda d: {(k[len("explore_model."):] if k.startswith("explore_model.") else k): v for k, v in d.items()}  # noqa: E731
    f = lambda d: {k: torch.as_tensor(np.asarray(strip(d)[k]), dtype=torch.float32).clone() for k in NAMES}  # noqa: E731
    sd = f(sd)
    return dict(sd=sd, target=f(target) if target is not None else {k: v.clone() for k, v in sd.items()},
                m={k: torch.zeros_like(sd[k]) for k in NAMES}, v={k: torch.zeros_like(sd[k]) for k in NAMES}, step=0)


def sync_target(state):
    state["target"] = {k: v.clone() for k, v in state["sd"].items()}


def fp32_train_step(state, batch, discount=0.5, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, update=True):
    st, ast, act, rw, nst, nast, dn = _t(batch)
    p = {k: state["sd"][k].clone().requires_grad_(True) for k in NAMES}
    tg = state["target"]

    def net(w, x, a):
        return (torch.cat([x, a], dim=1) @ w[W1].T + w[B1]) @ w[W2].T + w[B2]
    rows = torch.arange(len(rw))
    with torch.no_grad():
        new_qs = rw + discount * net(tg, nst, nast).max(dim=1).values * ~dn
        target_qs = net(p, st, ast).clone()
        target_qs[rows, act[:, 0].clamp(0, 2)] = new_qs  # (the clamp is the device contract's: the reference would raise)
    loss = torch.nn.functional.mse_loss(net(p, st, ast), target_qs)
    loss.backward()
    grads = {k: p[k].grad.detach().clone() for k in NAMES}
    if update:
        adam(state, grads, lr, betas, eps)
    return float(loss.detach()), grads


def contract_hidden(w, x, a):
    """layer1 as the device computes it: [B, 32] fp32."""
    F = x.shape[1]
    acc = (bf16(x).double() @ bf16(w[W1][:, :F]).double().T).to(torch.float32)
    wa, aa = bf16(w[W1][:, F:]), bf16(a)
    return acc + (aa[:, 0:1] * wa[:, 0] + aa[:, 1:2] * wa[:, 1]) + w[B1]


def contract_forward(state, batch, discount=0.5):
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd, tg = state["sd"], state["target"]
    h, hn = contract_hidden(sd, st, ast), contract_hidden(tg, nst, nast)
    lin = lambda v, w, b: (v.double() @ w.double().T).to(torch.float32) + b  # noqa: E731
    q, qn = lin(h, sd[W2], sd[B2]), lin(hn, tg[W2], tg[B2])
    a = act[:, 0].clamp(0, 2)
    y = rw + discount * qn.max(dim=1).values * (~dn).to(torch.float32)
    return dict(h=h, hn=hn, q=q, qn=qn, a=a, d=q[torch.arange(len(rw)), a] - y, xe=bf16(torch.cat([st, ast], 1)))


def contract_backward(state, f):
    """From contract_forward's f, in fp32: dq [B, 4] (dL/dq at the taken action, then the row's loss term) and
    dh [B, 32] = dq w2[a], one product per element."""
    d, a = f["d"], f["a"]
    B = len(d)
    scale, inv = float(np.float32(2.0 / (3.0 * B))), float(np.float32(1.0 / (3.0 * B)))
    g = d * scale
    dq = torch.zeros((B, 4), dtype=torch.float32)
    dq[torch.arange(B), a] = g
    dq[:, 3] = d * d * inv
    return dq, g[:, None] * state["sd"][W2][a]


def contract_train_step(state, batch, discount=0.5, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, update=True):
    f = contract_forward(state, batch, discount)
    h = f["h"]
    dq, dh = contract_backward(state, f)
    loss = float(dq[:, 3].double().sum())
    dq = dq[:, :3]
    grads = {W1: (dh.double().T @ f["xe"].double()).to(torch.float32), B1: dh.double().sum(0).to(torch.float32),
             W2: (dq.double().T @ h.double()).to(torch.float32), B2: dq.double().sum(0).to(torch.float32)}
    if update:
        adam(state, grads, lr, betas, eps)
    return loss, grads


def _bounds(state, batch, discount, h, hn, eh, ehn, xe, exe, own, elem, rowsum, loss_elem):
    """A forward error bound carried to the loss and to every gradient.  h, hn: the hidden values of the rows (under the
    model) and of their successors (under the target), eh, ehn what they may be off by; xe [B, F + 2] the layer1
    gradient's right operand and exe what IT may be off by (float64).  Layer2 is dqn_ref.propagate_head's head (e_q, e_y,
    e_d, the loss, g_w2, g_b2); from its d and e_d, layer1:
        dh:    e_dh[b][j] = 2 / (3 B) (e_d + elem (|d| + e_d)) |w2[a][j]|    d's error through w2[a]; elem: the scaling and
                                                                              the product dq * w2 round once each
        g_w1:  sum_b (e_dh (|xe| + e_xe) + |dh| e_xe)  +  rowsum sum_b (|dh| + e_dh) (|xe| + e_xe)
        g_b1:  the same with xe := 1, e_xe := 0.
    Key "dh" holds e_dh."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd, tg = state["sd"], state["target"]
    a = act[:, 0].clamp(0, 2)
    out = {}
    out["loss"], out[W2], out[B2], d, ed = D.propagate_head(sd[W2], sd[B2], tg[W2], tg[B2], a, rw, (~dn).double(), discount,
                                                            h, hn, eh, ehn, own, elem, rowsum, loss_elem)
    c = 2.0 / (3 * len(rw))
    wa = sd[W2].double()[a].abs()                                        # [B, 32]
    dh = c * d.abs()[:, None] * wa
    edh = c * (ed + elem * (d.abs() + ed))[:, None] * wa
    out[W1] = edh.T @ (xe.abs() + exe) + dh.T @ exe + rowsum * ((dh + edh).T @ (xe.abs() + exe))
    out[B1] = edh.sum(0) + rowsum * (dh + edh).sum(0)
    out["dh"] = edh  # [B, 32]: what dh itself may be off by
    return out


def bf16_bounds(state, batch, discount=0.5):
    """How far the contract may stand from fp32, from bfloat16's unit roundoff u = 2^-9 alone.  x and w1 are each rounded
    once in the forward, so a product is off by at most (2 u + u^2) |x w|: e_h = (2 u + u^2) (|x| |w1|^T); the layer1
    gradient's x is rounded once: e_xe = u |x|.  d, h taken from the fp32 forward; fp32 summation adds 2^-24-sized terms
    on top, far below (fp32_sum_bounds)."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd, tg = state["sd"], state["target"]
    c = 2 * U_BF16 + U_BF16 ** 2
    x, xn = torch.cat([st, ast], 1).double(), torch.cat([nst, nast], 1).double()
    eh, ehn = c * (x.abs() @ sd[W1].double().abs().T), c * (xn.abs() @ tg[W1].double().abs().T)
    h, hn = x @ sd[W1].double().T + sd[B1].double(), xn @ tg[W1].double().T + tg[B1].double()
    return _bounds(state, batch, discount, h, hn, eh, ehn, x, U_BF16 * x.abs(), 0.0, 0.0, 0.0, 0.0)


def fp32_sum_bounds(state, batch, discount=0.5):
    """An a-priori bound on |device - contract_train_step| per tensor (elementwise, float64) and for the loss (key
    "loss"), from the order of fp32 sums alone; nothing is read from a device.  Operands are equal on both sides (the
    bfloat16 roundings are part of the contract), so all that differs is where sums round.  With u = 2^-24:
        layer1   e_h = gamma(F + 3) (|bf16 x| |bf16 w1|^T + |b1|)     under the model for h, the target for h'
        layer2   that error through |w2|, and gamma(34) on its own sum of 32 products and a bias
        y, d     4 u on the operands (discount * max, + reward, q - y, the restatement's own rounding)
        dh       d's error through w2[a]; 4 u for the two roundings of d * scale * w2[a][j] on either side
        rows     gamma(B + 2) sum_b |term| for g_w2, g_b2, g_w1, g_b1 alike: B - 1 additions, the product, the
                 restatement's rounding (bf16 x is exact on both sides: e_xe = 0)
        loss     gamma(4) more per term."""
    h, hn, eh, ehn, xe = _sum_bound_hidden(state, batch)
    return _bounds(state, batch, discount, h, hn, eh, ehn, xe, torch.zeros_like(xe), gamma(34), 4 * U_FP32,
                   gamma(len(batch[3]) + 2), gamma(4))


def _sum_bound_hidden(state, batch):
    """Layer1 under fp32_sum_bounds: h, h', what they may be off by, and xe (float64)."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    F = st.shape[1]

    def hidden(w, x, a):
        xa = bf16(torch.cat([x, a], 1)).double()
        w1, b1 = bf16(w[W1]).double(), w[B1].double()
        return xa, xa @ w1.T + b1, gamma(F + 3) * (xa.abs() @ w1.abs().T + b1.abs())
    (xe, h, eh), (_, hn, ehn) = hidden(state["sd"], st, ast), hidden(state["target"], nst, nast)
    return h, hn, eh, ehn, xe


# ---- the workspace (antsrl_exptrain.hip): the forward stage's partials, then dh ---------------------------------------------
OUT = 100   # what a workgroup of the forward stage sums over its rows: layer2's 99 gradients (w2 [3][32], b2 [3]), the loss
PART = 104  # floats per workgroup in the workspace: OUT and four of padding


def blocks(B):
    """Workgroups of the forward stage (antsrl_exptrain_blocks): four tiles of 32 rows each, one per wave, no looping."""
    return ((B + 31) // 32 + 3) // 4


def work_layout(B):
    """The workspace of a step on B rows: partials [blocks][PART] fp32 from byte 0, dh [B][32] fp32 at the next multiple
    of 256 bytes, nothing behind row B - 1."""
    dh = (blocks(B) * PART * 4 + 255) // 256 * 256
    return dict(blocks=blocks(B), dh_offset=dh, bytes=dh + B * 32 * 4)


def row_workgroup(B):
    """[B] int64: tile t = b // 32 belongs to workgroup t // 4 (wave t % 4)."""
    return torch.arange(B) // 128


def row_terms(dq, h):
    """dq [B, 4] (contract_backward's) and h [B, 32] -> [B, OUT]: what each row adds to the forward stage's outputs."""
    B = len(dq)
    h1 = torch.cat([h, torch.ones((B, 1), dtype=h.dtype)], 1)
    return torch.cat([(dq[:, :3, None] * h1[:, None, :32]).reshape(B, 96), dq], 1)


def device_order_sum(terms, B):
    """terms [B, n] fp32 -> ([n], [blocks, n]): the row sums in the order of k_exptrain_fwd and the last workgroup of
    k_exptrain_l1, and the workgroups' partials on the way (a wave's one tile row by row from zero, the workgroup's
    four waves, then the workgroups)."""
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


def ordered_sum(part):
    """[blocks, n] fp32 -> [n]: a sequential fp32 sum from 0.0 in workgroup order."""
    s = torch.zeros((part.shape[1],), dtype=torch.float32)
    for b in range(part.shape[0]):
        s = s + part[b]
    return s


def expected_partials(state, batch, discount=0.5):
    """[blocks, OUT] float64: every workgroup's partial from contract_forward's h and d, the products and the sums over
    the workgroup's rows in float64."""
    f = contract_forward(state, batch, discount)
    B = len(f["d"])
    dq, _ = contract_backward(state, f)
    return torch.zeros((blocks(B), OUT), dtype=torch.float64).index_add_(0, row_workgroup(B), row_terms(dq.double(), f["h"].double()))


def partial_bounds(state, batch, discount=0.5):
    """fp32_sum_bounds' layer2 and loss for one workgroup's partial at a time, [blocks, OUT] float64: the terms summed over
    that workgroup's rows only, with the batch's B in 2 / (3 B) and 1 / (3 B), and gamma(rows + 4 + 2) for the row sums,
    rows being the workgroup's (the rows, the wave adds, the product and the restatement's rounding)."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    sd, tg = state["sd"], state["target"]
    B = len(rw)
    h, hn, eh, ehn, _ = _sum_bound_hidden(state, batch)
    group = row_workgroup(B)
    rowsum = gamma(torch.bincount(group, minlength=blocks(B)).double() + 6)
    loss, gw, gb = D.propagate_head_grouped(sd[W2], sd[B2], tg[W2], tg[B2], act[:, 0].clamp(0, 2), rw, (~dn).double(), discount,
                                            h, hn, eh, ehn, group, rowsum, own=gamma(34), elem=4 * U_FP32, loss_elem=gamma(4))[:3]
    return torch.cat([gw.reshape(-1, 96), gb, loss[:, None]], 1)


#: (F, B) at which the workspace is read back (test_gpu_dqn_train_workspace.py): two tiles in one workgroup, five
#: workgroups narrow and at F = 294, the cap of 512 workgroups narrow and at F = 294, the widest rows
WORKSPACE_SHAPES = ((17, 33), (17, 513), (294, 513), (17, 65536), (294, 65536), (1022, 33))


def workspace_case(F, B):
    """make_case at a WORKSPACE_SHAPES shape (a ring of 3000 rows under the large batches)."""
    return make_case(F, B, 100 * F + B, N=3000 if B > 4096 else None)


# ---- the cases both test files share -----------------------------------------------------------------------------------
def make_case(F, B, seed, N=None, dones="some", spread=True):
    """A net (model and a target that differs from it), a replay of N rows and B indices into it, on the CPU.
    Observations are sparse and non-negative as the environment's are; agent_state in [-2, 2); rewards ~ N(0, 1);
    weights are nn.Linear's init scaled up 3 x in layer2 so that dh, and with it layer1's gradient, is not small against
    layer2's.  Returns (state, arrays, idx)."""
    g = torch.Generator().manual_seed(seed)
    N = N or max(3 * B // 2 + 7, 40)
    IN = F + 2

    def net():
        u = lambda shape, b: (torch.rand(shape, generator=g) * 2 - 1) * b  # noqa: E731
        return {W1: u((32, IN), IN ** -0.5), B1: u((32,), IN ** -0.5), W2: u((3, 32), 3 * 32 ** -0.5), B2: u((3,), 32 ** -0.5)}
    state = new_state(net(), net())
    st, nst = torch.rand((N, F), generator=g), torch.rand((N, F), generator=g)
    st[torch.rand((N, F), generator=g) < 0.5] = 0.0
    nst[torch.rand((N, F), generator=g) < 0.5] = 0.0
    ast, nast = torch.rand((N, 2), generator=g) * 4 - 2, torch.rand((N, 2), generator=g) * 4 - 2
    act = torch.stack([torch.randint(0, 3, (N,), generator=g), torch.ones((N,), dtype=torch.int64)], 1)
    rw = torch.randn((N,), generator=g)
    dn = {"some": torch.rand((N,), generator=g) < 0.3, "all": torch.ones((N,), dtype=torch.bool),
          "none": torch.zeros((N,), dtype=torch.bool)}[dones]
    idx = torch.randint(0, N, (B,), generator=g)
    return state, (st, ast, act, rw, nst, nast, dn), idx


#: (F, B): the smallest shapes at which each seam of antsrl_exptrain.hip exists — one row, a partial and a full 32-row
#: tile, more than one tile / wave / workgroup of the forward stage (4 tiles each), F below one k-step, F not a multiple
#: of 4, 8 or 16, a column slab that straddles states | agent_state | bias, the widths around 608 (where a design with one
#: LDS image at a time would switch), the widest rows, and a batch of many workgroups
SHAPES = ((1, 1), (1, 33), (17, 31), (17, 32), (17, 33), (17, 513), (294, 256), (294, 512), (294, 513), (607, 33), (608, 33),
          (609, 33), (1022, 33), (1022, 256), (17, 4096))
#: further cases at F = 17, B = 40: name -> (make_case keywords, discount)
VARIANTS = {"idx_null": ({}, 0.5), "idx_clamped": ({}, 0.5), "actions_clamped": ({}, 0.5), "dones_all": (dict(dones="all"), 0.5),
            "dones_none": (dict(dones="none"), 0.5), "discount_0": ({}, 0.0), "discount_0.99": ({}, 0.99),
            "nan_ring": ({}, 0.5)}


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
