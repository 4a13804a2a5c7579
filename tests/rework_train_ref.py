"""The rework agent's training step restated, for the tests of antsrl_reworktrain_step.  CPU only.

  autograd_step        CollectAgentRework.train (agents/collect_agent_rework.py:110-152) for CollectModelRework (:24-63) in
                       torch autograd on the CPU, float32 (the reference's own arithmetic) or float64 (the yardstick);
  fp32_train_step      the float32 one followed by torch.optim.Adam's single-tensor update (dqn_ref.adam);
  down_chain, batch_pass, contract
                       the device contract of include/antsrl.h: the head rows pushed down (M_l) and the pseudo-rows pushed
                       up (A_l) in float64 in the device's order of sums, every gradient sum_k M_l[k] (x) A_in(l)[k] rounded
                       once; `contract` takes G and s as given (the device's own, in the device tests), `batch_pass` makes
                       them in float32 without claiming the device's order of the row sums;
  rank_step            the three together: the whole step in the rank-NQ form.

`state`: sd (the 20 tensors under CollectModelRework's names), target (the same 20), m / v (Adam's moments), step.
`batch` = (states [B, F], agent_states [B, 2], actions [B, 2], rewards [B], new_states, new_agent_states, dones [B]),
already gathered.  Steps return (loss, grads by name)."""
import math
from functools import partial

import numpy as np
import torch

import dqn_ref as D
import rework_policy_ref as R
from dqn_ref import U_FP32, gather  # noqa: F401
from dqn_ref import as_batch as _t

LAYERS = R.LAYERS
NAMES = tuple(l + s for l in LAYERS for s in (".weight", ".bias"))
#: the layer that feeds layer l (None: x)
SRC = dict(layer1=None, layer2="layer1", layer3="layer2", layer4="layer3", rotation_layer1="layer4",
           rotation_layer2="rotation_layer1", rotation_layer3="rotation_layer2", rotation_layer4="rotation_layer3",
           pheromone_layer1="layer4", pheromone_layer2="pheromone_layer1")
#: the layers whose A the gradient needs, in the order the up chain makes them
UP_ROT = ("layer1", "layer2", "layer3", "layer4", "rotation_layer1", "rotation_layer2", "rotation_layer3")
UP_PH = ("layer1", "layer2", "layer3", "layer4", "pheromone_layer1")
A_LAYERS = ("layer1", "layer2", "layer3", "layer4", "rotation_layer1", "rotation_layer2", "rotation_layer3", "pheromone_layer1")
adam = partial(D.adam, NAMES)
#: the floor of the accuracy bound, in units of 2^-24 of the tensor's largest float64 gradient (C_FLOOR) and of the float64
#: loss (C_FLOOR_LOSS): four times the rank form's worst error on the CPU over CASES and VARIANTS, taken over the
#: quantities whose error exceeds the reference's own float32 one (elsewhere e_ref is the larger term of the bound and the
#: floor plays no part: a bias gradient whose rows cancel is 180 units off in the rank form and 1500 in torch's float32).
#: The worst were 4.24 and 4.55; test_rework_train_fixture.py checks that a CPU's worst stays within a quarter above.
C_FLOOR = 17.0
C_FLOOR_LOSS = 18.3


def new_state(sd, target=None):
    f = lambda d: {k: torch.as_tensor(np.asarray(d[k]), dtype=torch.float32).clone() for k in NAMES}  # noqa: E731
    sd = f(sd)
    return dict(sd=sd, target=f(target) if target is not None else {k: v.clone() for k, v in sd.items()},
                m={k: torch.zeros_like(sd[k]) for k in NAMES}, v={k: torch.zeros_like(sd[k]) for k in NAMES}, step=0)


def sync_target(state):
    state["target"] = {k: v.clone() for k, v in state["sd"].items()}


def heads(sd):
    return sd["rotation_layer4.bias"].shape[0], sd["pheromone_layer2.bias"].shape[0]


def _clamped_actions(act, n_rot, n_ph):
    """(the clamp is the device contract's: the reference would raise)"""
    return act[:, 0].clamp(0, n_rot - 1), act[:, 1].clamp(0, n_ph - 1)


def autograd_step(state, batch, dtype=torch.float32, discount=0.5):
    st, ast, act, rw, nst, nast, dn = _t(batch)
    n_rot, n_ph = heads(state["sd"])
    p = {k: state["sd"][k].to(dtype).clone().requires_grad_(True) for k in NAMES}
    tg = {k: v.to(dtype) for k, v in state["target"].items()}
    B = len(rw)
    rows = torch.arange(B)
    ar, ap = _clamped_actions(act, n_rot, n_ph)

    def net(w, s, a):
        x = torch.cat([s.to(dtype), a.to(dtype)], dim=1)
        lin = lambda n, t: torch.nn.functional.linear(t, w[n + ".weight"], w[n + ".bias"])  # noqa: E731
        g = lin("layer4", lin("layer3", lin("layer2", lin("layer1", x))))
        return (lin("rotation_layer4", lin("rotation_layer3", lin("rotation_layer2", lin("rotation_layer1", g)))),
                lin("pheromone_layer2", lin("pheromone_layer1", g)))
    with torch.no_grad():
        f_rot, f_ph = net(tg, nst, nast)
        t_rot, t_ph = (t.clone() for t in net(p, st, ast))
        live = (~dn).to(dtype)
        t_rot[rows, ar] = rw.to(dtype) + discount * f_rot.max(dim=1).values * live
        t_ph[rows, ap] = rw.to(dtype) + discount * f_ph.max(dim=1).values * live
    q_rot, q_ph = net(p, st, ast)
    loss = torch.nn.functional.mse_loss(q_rot, t_rot) + torch.nn.functional.mse_loss(q_ph, t_ph)
    loss.backward()
    return float(loss.detach()), {k: p[k].grad.detach().clone() for k in NAMES}


def fp32_train_step(state, batch, discount=0.5, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, update=True):
    loss, grads = autograd_step(state, batch, torch.float32, discount)
    if update:
        adam(state, grads, lr, betas, eps)
    return loss, grads


# ---- the device contract ---------------------------------------------------------------------------------------------
def _f64(sd):
    return {k: torch.as_tensor(v).detach().cpu().numpy().astype(np.float32).astype(np.float64) for k, v in sd.items()}


def _push_down(v, W):
    """v [n, out] through W [out][in]: ((0 + v[:, 0] W[0]) + v[:, 1] W[1]) + ..., every product rounded."""
    acc = np.zeros((v.shape[0], W.shape[1]))
    for i in range(W.shape[0]):
        acc = acc + v[:, i:i + 1] * W[i][None, :]
    return acc


def down_chain(sd):
    """{layer: M_l float64 [NQ, out_l]} as k_reworktrain_down stores them: a head's last layer holds the unit rows, every
    layer below it the rows pushed down so far (rework_policy_ref.collapse64's v on its way), the other head's own layers
    zeros."""
    P = _f64(sd)
    n_rot, n_ph = heads(sd)
    NQ = n_rot + n_ph
    M = {l: np.zeros((NQ, P[l + ".bias"].shape[0])) for l in LAYERS}
    for last, chain, rows in (("rotation_layer4", R.ROT_CHAIN, slice(0, n_rot)), ("pheromone_layer2", R.PH_CHAIN, slice(n_rot, NQ))):
        M[last][rows] = np.eye(P[last + ".bias"].shape[0])
        v = P[last + ".weight"].copy()
        for l in chain:
            M[l][rows] = v
            v = _push_down(v, P[l + ".weight"])
    return M


def batch_pass(state, batch, discount=0.5):
    """(G float32 [NQ, D], s float32 [NQ], loss) from the two collapsed nets in float32: the batch's part of the step.
    The order of the sums over the rows is torch's, not the device's."""
    st, ast, act, rw, nst, nast, dn = _t(batch)
    n_rot, n_ph = heads(state["sd"])
    B = len(rw)
    (wc, bc), (twc, tbc) = R.collapse64(state["sd"]), R.collapse64(state["target"])
    x, xn = torch.cat([st, ast], 1), torch.cat([nst, nast], 1)
    q, qn = x @ wc.T + bc, xn @ twc.T + tbc
    rows = torch.arange(B)
    ar, ap = _clamped_actions(act, n_rot, n_ph)
    live = (~dn).to(torch.float32)
    d_rot = q[rows, ar] - (rw + discount * qn[:, :n_rot].max(dim=1).values * live)
    d_ph = q[rows, n_rot + ap] - (rw + discount * qn[:, n_rot:].max(dim=1).values * live)
    dq = torch.zeros((B, n_rot + n_ph), dtype=torch.float32)
    dq[rows, ar] = d_rot * float(np.float32(2.0 / (n_rot * B)))
    dq[rows, n_rot + ap] = d_ph * float(np.float32(2.0 / (n_ph * B)))
    loss = float((d_rot * d_rot).sum() * np.float32(1.0 / (n_rot * B)) + (d_ph * d_ph).sum() * np.float32(1.0 / (n_ph * B)))
    return dq.T @ x, dq.sum(0), loss


def contract(sd, G, s, M=None):
    """(A {layer: float64 [NQ, out_l]}, grads {name: float32 tensor}) from G [NQ, D] and s [NQ] (float32) in the device's
    order: A_l[k][j] = ((0 + A_in[k][0] W[j][0]) + A_in[k][1] W[j][1]) + ... + s[k] b[j], the rows of the other head zero;
    gradient (float)(((0 + M_l[k0][o] A_in[k0][c]) + ...) over the pseudo-rows of l's head, s[k] in A's place for a bias."""
    P = _f64(sd)
    n_rot, n_ph = heads(sd)
    NQ = n_rot + n_ph
    M = down_chain(sd) if M is None else M
    G = np.asarray(G, dtype=np.float32).astype(np.float64)
    s = np.asarray(s, dtype=np.float32).astype(np.float64)
    A = {l: np.zeros((NQ, P[l + ".bias"].shape[0])) for l in A_LAYERS}
    for chain, rows in ((UP_ROT, slice(0, n_rot)), (UP_PH, slice(n_rot, NQ))):
        cur = G[rows]
        for l in chain:
            W, b = P[l + ".weight"], P[l + ".bias"]
            acc = np.zeros((cur.shape[0], W.shape[0]))
            for c in range(W.shape[1]):
                acc = acc + cur[:, c:c + 1] * W[:, c][None, :]
            acc = acc + s[rows][:, None] * b[None, :]
            A[l][rows] = acc
            cur = acc
    grads = {}
    for l in LAYERS:
        general = not (l.startswith("rotation") or l.startswith("pheromone"))
        ks = range(NQ) if general else (range(n_rot) if l.startswith("rotation") else range(n_rot, NQ))
        Ain = G if SRC[l] is None else A[SRC[l]]
        gw, gb = np.zeros_like(P[l + ".weight"]), np.zeros_like(P[l + ".bias"])
        for k in ks:
            gw = gw + M[l][k][:, None] * Ain[k][None, :]
            gb = gb + M[l][k] * s[k]
        grads[l + ".weight"] = torch.from_numpy(gw.astype(np.float32))
        grads[l + ".bias"] = torch.from_numpy(gb.astype(np.float32))
    return A, grads


def rank_step(state, batch, discount=0.5):
    G, s, loss = batch_pass(state, batch, discount)
    return loss, contract(state["sd"], G, s)[1]


# ---- errors and the accuracy bound -----------------------------------------------------------------------------------
def tensor_errors(g, g64):
    """{name: max |g - g64|} (float)."""
    return {k: float((g[k].double() - g64[k].double()).abs().max()) for k in NAMES}


def accuracy_bounds(state, batch, discount=0.5):
    """What the device's gradients and loss are held to: per tensor 4 max(e_ref, floor), e_ref = max |g32 - g64|
    of the reference's own float32 autograd on these rows and weights, floor = C_FLOOR 2^-24 max |g64|; the loss likewise with C_FLOOR_LOSS.
    Returns (bounds by name and "loss", g64, loss64)."""
    l64, g64 = autograd_step(state, batch, torch.float64, discount)
    l32, g32 = autograd_step(state, batch, torch.float32, discount)
    e = tensor_errors(g32, g64)
    bd = {k: 4.0 * max(e[k], C_FLOOR * U_FP32 * float(g64[k].abs().max())) for k in NAMES}
    bd["loss"] = 4.0 * max(abs(l32 - l64), C_FLOOR_LOSS * U_FP32 * abs(l64))
    return bd, g64, l64


def floor_ratios(state, batch, discount=0.5):
    """The rank form's errors against float64 in units of 2^-24 of the tensor's largest gradient (of the loss), where they
    exceed the reference's own float32 error (0 where none does): (worst over the tensors, the loss's)."""
    l64, g64 = autograd_step(state, batch, torch.float64, discount)
    l32, g32 = autograd_step(state, batch, torch.float32, discount)
    loss, g = rank_step(state, batch, discount)
    e, e_ref = tensor_errors(g, g64), tensor_errors(g32, g64)
    return (max([e[k] / (U_FP32 * float(g64[k].abs().max())) for k in NAMES if e[k] > e_ref[k]] + [0.0]),
            abs(loss - l64) / (U_FP32 * abs(l64)) if abs(loss - l64) > abs(l32 - l64) else 0.0)


# ---- the workspace (antsrl_reworktrain.h) ----------------------------------------------------------------------------
ROWS = 16        # rows a workgroup of the batch pass takes at a time, four per wave
MAX_PARTS = 256


def widths(sd):
    return {l: tuple(sd[l + ".weight"].shape) for l in LAYERS}  # (out, in)


def work_layout(sd, B):
    """Byte offsets of the workspace of a step on B rows for the net sd, every part rounded up to 256 bytes (include/antsrl.h):
    collapsed, M[layer], partials ([parts][stride] floats), G (then s), A[layer]; parts, stride, bytes."""
    n_rot, n_ph = heads(sd)
    NQ, Dm = n_rot + n_ph, sd["layer1.weight"].shape[1]
    out = {l: sd[l + ".bias"].shape[0] for l in LAYERS}
    at = [0]

    def take(n):
        here = at[0]
        at[0] += (n + 255) // 256 * 256
        return here
    L = dict(parts=min((B + ROWS - 1) // ROWS, MAX_PARTS), stride=(NQ * Dm + NQ + 2 + 63) // 64 * 64)
    L["collapsed"] = take(4 * (NQ * Dm + NQ))
    L["M"] = {l: take(8 * NQ * out[l]) for l in LAYERS}
    L["partials"] = take(4 * L["parts"] * L["stride"])
    L["G"] = take(4 * (NQ * Dm + NQ))
    L["A"] = {l: take(8 * NQ * out[l]) for l in A_LAYERS}
    L["bytes"] = at[0]
    return L


def ordered_sum(part):
    """[parts, n] fp32 -> [n]: a sequential fp32 sum from 0.0 in workgroup order."""
    s = torch.zeros((part.shape[1],), dtype=torch.float32)
    for b in range(part.shape[0]):
        s = s + part[b]
    return s


def read_workspace(work, sd, B):
    """The workspace bytes (uint8 on the CPU) of a step on B rows as named arrays: collapsed (Wc, bc), M, partials, G, s, A."""
    n_rot, n_ph = heads(sd)
    NQ, Dm = n_rot + n_ph, sd["layer1.weight"].shape[1]
    L = work_layout(sd, B)
    out = {l: sd[l + ".bias"].shape[0] for l in LAYERS}
    f32 = lambda o, n: work[o: o + 4 * n].view(torch.float32).clone()  # noqa: E731
    f64 = lambda o, n: work[o: o + 8 * n].view(torch.float64).clone()  # noqa: E731
    col, gs = f32(L["collapsed"], NQ * Dm + NQ), f32(L["G"], NQ * Dm + NQ)
    return dict(Wc=col[: NQ * Dm].view(NQ, Dm), bc=col[NQ * Dm:], G=gs[: NQ * Dm].view(NQ, Dm), s=gs[NQ * Dm:],
                M={l: f64(L["M"][l], NQ * out[l]).view(NQ, out[l]) for l in LAYERS},
                A={l: f64(L["A"][l], NQ * out[l]).view(NQ, out[l]) for l in A_LAYERS},
                partials=f32(L["partials"], L["parts"] * L["stride"]).view(L["parts"], L["stride"])[:, : NQ * Dm + NQ + 2].clone(),
                layout=L)


# ---- cases -----------------------------------------------------------------------------------------------------------
DEFAULT_HIDDEN = dict(g=(64, 128, 32), r=(64, 128, 32), p1=32)
ODD_HIDDEN = dict(g=(5, 7, 3), r=(256, 1, 9), p1=1)


def param_shapes(F, n_rot, n_ph, g=(64, 128, 32), r=(64, 128, 32), p1=32):
    Dm = F + 2
    return dict(layer1=(g[0], Dm), layer2=(g[1], g[0]), layer3=(g[2], g[1]), layer4=(Dm, g[2]), rotation_layer1=(r[0], Dm),
                rotation_layer2=(r[1], r[0]), rotation_layer3=(r[2], r[1]), rotation_layer4=(n_rot, r[2]),
                pheromone_layer1=(p1, Dm), pheromone_layer2=(n_ph, p1))


def make_case(F, B, seed, n_rot=3, n_ph=3, hidden=None, model="spread", N=None, dones="some"):
    """A net (model and a target that differs from it), a replay of N rows and B indices into it (with replacement: some
    repeat), on the CPU.  Weights: nn.Linear's init under the seed, in rework_policy_ref's two scalings (`spread`: weights
    x 3, biases x 0.1; `init`: as constructed).  Observations as rework_policy_ref.synthetic's (sparse, up to 255, exact in
    bfloat16), agent_state in [0, 1), rewards in [-0.5, 1.5), 10 % dones (or all, or none).  Returns (state, arrays, idx)."""
    g = torch.Generator().manual_seed(seed)
    N = N or max(3 * B // 2 + 7, 40)
    wf, bf = (3.0, 0.1) if model == "spread" else (1.0, 1.0)

    def net():
        sd = {}
        for name, (o, i) in param_shapes(F, n_rot, n_ph, **(hidden or {})).items():
            b = 1.0 / math.sqrt(i)
            sd[name + ".weight"] = (torch.rand((o, i), generator=g) * 2 - 1) * b * wf
            sd[name + ".bias"] = (torch.rand((o,), generator=g) * 2 - 1) * b * bf
        return sd
    state = new_state(net(), net())

    def obs():
        val, pick = torch.rand((N, F), generator=g) * 255.0, torch.rand((N, F), generator=g) < 0.15
        return torch.where(pick, val, torch.zeros(())).to(torch.bfloat16).to(torch.float32)
    st, nst = obs(), obs()
    ast, nast = torch.rand((N, 2), generator=g), torch.rand((N, 2), generator=g)
    act = torch.stack([torch.randint(0, n_rot, (N,), generator=g), torch.randint(0, n_ph, (N,), generator=g)], 1)
    rw = torch.rand((N,), generator=g) * 2 - 0.5
    dn = {"some": torch.rand((N,), generator=g) < 0.1, "all": torch.ones((N,), dtype=torch.bool),
          "none": torch.zeros((N,), dtype=torch.bool)}[dones]
    idx = torch.randint(0, N, (B,), generator=g)
    return state, (st, ast, act, rw, nst, nast, dn), idx


#: name -> make_case keywords.  F = 9 and 294 give D = 11 and 296 (a ragged tail; 11 is below one 64-input chunk), 62 gives
#: D = 64 (exactly one chunk), 1022 the largest D.  A wave of the batch pass takes 4 rows, a workgroup 16: B = 1, 3, 4, 5,
#: 17; 264 is the reference's minibatch; 4113 needs all 256 partials and loops (258 passes).  Heads (1, 8) have NQ = 9: the
#: 16-output instance of the batch pass, and at F = 1022 its largest LDS image.  The odd hidden widths include 1 and 256.
CASES = {
    "F9_B1": dict(F=9, B=1), "F9_B3": dict(F=9, B=3), "F9_B4_init": dict(F=9, B=4, model="init"), "F9_B5": dict(F=9, B=5),
    "F9_B17_h18": dict(F=9, B=17, n_rot=1, n_ph=8), "F62_B17_h25": dict(F=62, B=17, n_rot=2, n_ph=5),
    "F62_B33_odd": dict(F=62, B=33, hidden=ODD_HIDDEN, model="init"), "F294_B264": dict(F=294, B=264),
    "F294_B264_init": dict(F=294, B=264, model="init"), "F294_B33_odd_h25": dict(F=294, B=33, hidden=ODD_HIDDEN, n_rot=2, n_ph=5),
    "F1022_B17": dict(F=1022, B=17), "F1022_B5_h18": dict(F=1022, B=5, n_rot=1, n_ph=8),
    "F9_B4113": dict(F=9, B=4113, N=3000), "F294_B4113_init": dict(F=294, B=4113, N=3000, model="init"),
}
#: further cases at F = 9, B = 40
VARIANTS = ("idx_null", "idx_duplicates", "idx_last_row", "idx_clamped", "actions_clamped", "dones_all", "dones_none")


def case(name):
    """(state, arrays, idx) of a CASES entry."""
    return make_case(seed=1 + sorted(CASES).index(name), **CASES[name])


def make_variant(name):
    """(state, arrays, idx or None, B) of a VARIANTS case; `arrays` is what the device gets, out-of-range values and all."""
    F, B = 9, 40
    kw = dict(dones="all") if name == "dones_all" else (dict(dones="none") if name == "dones_none" else {})
    state, arrays, idx = make_case(F, B, 500 + VARIANTS.index(name), **kw)
    N = arrays[0].shape[0]
    if name == "idx_null":  # without idx the minibatch is rows 0 .. B - 1 of the arrays
        arrays, idx = tuple(t[:B].clone() for t in arrays), None
    elif name == "idx_duplicates":
        idx[:] = idx[0]
        idx[1::3] = idx[1]
    elif name == "idx_last_row":
        idx[::4] = N - 1
    elif name == "idx_clamped":
        idx[::5] = torch.tensor([-1, N, -(1 << 40), 1 << 40, N + 3, -7, N, -1])
    elif name == "actions_clamped":
        arrays[2][::3, 0] = torch.tensor([-1, 3, 7, -(1 << 33), 1 << 33] * 20)[: len(arrays[2][::3])]
        arrays[2][1::3, 1] = torch.tensor([3, -1, 1 << 33, -(1 << 33), 9] * 20)[: len(arrays[2][1::3])]
    return state, arrays, idx, B


def gather_clamped(arrays, idx, B):
    """The minibatch rows as the device takes them: row idx[b] clamped to [0, N), or row b without idx."""
    N = arrays[0].shape[0]
    rows = torch.arange(B) if idx is None else idx.clamp(0, N - 1)
    return gather(arrays, rows)
