"""Test comparators for the memory agent's training step (CollectAgentMemory.train, agents/collect_agent_memory.py:133-176).
Test infrastructure only.

`fp32_train_step` restates train() in plain float32 PyTorch with autograd; tests/test_memory_train_fixture.py pins it
to tests/golden/contract/memory_train_ref.npz, i.e. to what the reference's own agent computed.  `bf16_train_grads` is
the same gradient by manual backprop at the rounding points of the kernel's precision contract (antsrl_memtrain.hip):
bf16 MFMA operands (layer inputs, weights, dOut, saved activations), everything else fp32.  `adam_step` restates
torch.optim.Adam's single-tensor arithmetic as the apply stage performs it.

The second half serves tests/test_gpu_memory_train_stages.py and tests/test_memory_train_bounds_cpu.py:
`state_layout` / `work_layout` restate antsrl_memtrain_state_layout / antsrl_memtrain_work_layout (include/antsrl.h), and
`stage_outputs` computes ONE launch of the grad stage from that launch's own inputs, in float64 with an a-priori fp32
bound per output element, or in fp32 (the CPU restatement, with or without a planted defect).
"""
import os

import numpy as np
import torch

from dqn_ref import RING, U_FP32, gamma  # noqa: F401
from memory_policy_ref import LAYERS, rebuild_seeded

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "memory_train_ref.npz")
TRAINED = LAYERS[:9]
TRAINED_KEYS = tuple(l + s for l in TRAINED for s in (".weight", ".bias"))
# layer -> the layer whose output is its input (None: x)
INPUT_OF = dict(layer1=None, layer2="layer1", layer3="layer2", layer4="layer3", rotation_layer1="layer4",
                rotation_layer2="rotation_layer1", rotation_layer3="rotation_layer2", pheromone_layer1="layer4",
                pheromone_layer2="pheromone_layer1")


def load_fixture():
    """-> (initial model state_dict rebuilt from the seed, the fixture's arrays)."""
    z = np.load(FIXTURE)
    rec = {k: z[k] for k in z.files}
    return rebuild_seeded(rec), rec


def fixture_batch(rec, c):
    """The minibatch of call c: (states, agent_states, actions, rewards, new_states, new_agent_states, dones) tensors."""
    pos = {int(r): i for i, r in enumerate(rec["rows/index"])}
    sel = np.array([pos[int(i)] for i in rec["c%d/idx" % c]])
    return tuple(torch.from_numpy(np.ascontiguousarray(rec["rows/" + k][sel])) for k in RING)


def _x(st, ast):
    B = st.shape[0]
    return torch.cat([st.reshape(B, -1).float(), ast.reshape(B, -1).float()], dim=1)


def fp32_train_step(sd, target_sd, batch, discount):
    """(loss, {name: grad}) of train()'s loss at weights sd, target net target_sd, in float32 with autograd (the
    reference's arithmetic: target q, TD target per head, MSE of the model's q against it, summed)."""
    st, ast, act, rw, nst, nast, dn = batch
    W = {k: v.detach().float().clone().requires_grad_(k in TRAINED_KEYS) for k, v in sd.items()}
    T = {k: v.detach().float() for k, v in target_sd.items()}

    def heads(P, s, a):
        x = _x(s, a)

        def lin(n, t):
            return t @ P[n + ".weight"].T + P[n + ".bias"]
        h = torch.relu(lin("layer1", x))
        h = torch.relu(lin("layer2", h))
        h = torch.relu(lin("layer3", h))
        g = lin("layer4", h) + x
        return (lin("rotation_layer3", lin("rotation_layer2", lin("rotation_layer1", g))),
                lin("pheromone_layer2", lin("pheromone_layer1", g)))
    with torch.no_grad():
        fr, fp = heads(T, nst, nast)
        tr, tp = heads(W, st, ast)
        rows = torch.arange(st.shape[0])
        nd = ~dn.bool()
        tr[rows, act[:, 0]] = rw + discount * fr.max(dim=1).values * nd
        tp[rows, act[:, 1]] = rw + discount * fp.max(dim=1).values * nd
    qr, qp = heads(W, st, ast)
    loss = torch.nn.functional.mse_loss(qr, tr) + torch.nn.functional.mse_loss(qp, tp)
    loss.backward()
    return loss.detach(), {k: W[k].grad for k in TRAINED_KEYS}


def bf16_train_grads(sd, target_sd, batch, discount, idx=None):
    """(loss, {name: grad}) at the kernel's rounding points: manual backprop with bf16 operands, fp32 elsewhere.
    Actions outside [0, n_head) contribute nothing.  Runs on the tensors' device."""
    st, ast, act, rw, nst, nast, dn = batch
    if idx is not None:
        st, ast, act, rw, nst, nast, dn = (t[idx] for t in batch)
    dev = st.device
    bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    M = {k: v.to(dev, torch.float32) for k, v in sd.items()}
    T = {k: v.to(dev, torch.float32) for k, v in target_sd.items()}

    def fwd(P, s, a):
        x = _x(s, a)
        out = {}

        def lin(n, t):
            return bf(t) @ bf(P[n + ".weight"]).T + P[n + ".bias"]
        out["layer1"] = torch.relu(lin("layer1", x))
        out["layer2"] = torch.relu(lin("layer2", out["layer1"]))
        out["layer3"] = torch.relu(lin("layer3", out["layer2"]))
        out["layer4"] = (bf(out["layer3"]) @ bf(P["layer4.weight"]).T + P["layer4.bias"]) + x
        for n in ("rotation_layer1", "rotation_layer2", "rotation_layer3", "pheromone_layer1", "pheromone_layer2"):
            out[n] = lin(n, out[INPUT_OF[n]])
        return x, out
    _, to = fwd(T, nst, nast)
    x, mo = fwd(M, st, ast)
    B = st.shape[0]
    nd = torch.where(dn.bool(), 0.0, 1.0).to(dev)
    loss = torch.zeros((), device=dev)
    dout = {}
    for head, key, col in (("rotation_layer3", "rotation_layer3", 0), ("pheromone_layer2", "pheromone_layer2", 1)):
        q, qt = mo[head], to[head]
        n = q.shape[1]
        a = act[:, col]
        ok = (a >= 0) & (a < n)
        y = rw + (_f32(discount) * qt.max(dim=1).values) * nd
        qa = q.gather(1, a.clamp(0, n - 1).view(-1, 1)).view(-1)
        d = torch.where(ok, qa - y, torch.zeros_like(y))
        loss = loss + (d * d * _f32(1.0 / (B * n))).sum()
        dq = torch.zeros_like(q)
        r = ok.nonzero().view(-1)
        dq[r, a[r]] = d[r] * _f32(2.0 / (B * n))
        dout[key] = dq

    def back(n):  # dOut of n's input: bf16 dOut . bf16 W
        return bf(dout[n]) @ bf(M[n + ".weight"])
    dout["rotation_layer2"] = back("rotation_layer3")
    dout["pheromone_layer1"] = back("pheromone_layer2")
    dout["rotation_layer1"] = back("rotation_layer2")
    dout["layer4"] = back("rotation_layer1") + back("pheromone_layer1")
    dout["layer3"] = back("layer4") * (mo["layer3"] > 0)
    dout["layer2"] = back("layer3") * (mo["layer2"] > 0)
    dout["layer1"] = back("layer2") * (mo["layer1"] > 0)
    grads = {}
    for n in TRAINED:
        inp = x if INPUT_OF[n] is None else mo[INPUT_OF[n]]
        grads[n + ".weight"] = bf(dout[n]).T @ bf(inp)
        grads[n + ".bias"] = dout[n].sum(dim=0)
    return loss, grads


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (single tensor, no weight decay) as the apply stage computes it, in float32 (-> new p, m, v);
    the scalars are derived in double and rounded to float, as torch does."""
    f = _f32
    bc1 = 1.0 - beta1 ** step
    bc2_sqrt = (1.0 - beta2 ** step) ** 0.5
    step_size = lr / bc1
    m = m + f(1.0 - beta1) * (g - m)
    v = v * f(beta2) + f(1.0 - beta2) * g * g
    denom = torch.sqrt(v) / f(bc2_sqrt) + f(eps)
    p = p + f(-step_size) * (m / denom)
    return p, m, v


def _f32(v):
    """v rounded to float32, as a Python scalar (what a torch op does with a double scalar on a float32 tensor)."""
    return float(np.float32(v))


def cosine(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp(min=1e-300))


# ======================================================================================================================
# The layouts of include/antsrl.h, restated (pinned to antsrl_memtrain_sizes by tests/test_memory_train_bounds_cpu.py)
# ======================================================================================================================
IN_OF = (-1, 0, 1, 2, 3, 4, 5, 3, 7)   # trained layer -> the trained layer whose output is its input (-1: x)
FWD_LAUNCH = ((0,), (1,), (2,), (3,), (4, 7), (5, 8), (6,))   # the layers of the 7 forward launches (both nets each)
BWD_LAUNCH = ((6, 8), (5,), (4,), (3,), (2,), (1,))           # dOut of these layers -> dOut of their input layer
DOUT_ORDER = (0, 1, 2, 3, 4, 5, 6, 7, 8)                      # dh1 dh2 dh3 dg dr1 dr2 dqr dp1 dqp = dOut of layer 0..8
STAGES = tuple("fwd%d" % i for i in range(7)) + ("td",) + tuple("bwd%d" % i for i in range(6)) + ("wgrad", "finalize")
TINY = 2.0 ** -126  # the smallest normal float: an MFMA may flush a subnormal product or sum


def _r(v, a):
    return (v + a - 1) // a * a


def layer_dims(F, power, mem, n_rot, n_ph):
    """The 13 layers (out, in) in state_dict order."""
    D, h1, h2, h3 = F + 2 + mem, 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power)
    return [(h2, D), (h3, h2), (h1, h3), (D, h1), (h2, D), (h3, h2), (n_rot, h3), (h1, D), (n_ph, h1),
            (h2, D), (h2, h2), (mem, h2), (mem, h2)]


def state_layout(F, power, mem, n_rot, n_ph):
    """A net's state buffer: params at 0, m, v, then the bf16 packs (W [Np][Kp] then W^T [Kp][Np] per trained layer)."""
    layers = layer_dims(F, power, mem, n_rot, n_ph)
    L = dict(out=[o for o, _ in layers], inn=[i for _, i in layers], poff=[], woff=[], wtoff=[])
    off = 0
    for l, (o, i) in enumerate(layers):
        L["poff"].append(off)
        off += o * i + o
        if l == 8:
            L["trained_floats"] = off
    L["params_floats"] = off
    L["Np"], L["Kp"] = [_r(o, 32) for o, _ in layers[:9]], [_r(i, 32) for _, i in layers[:9]]
    pe = 0
    for l in range(9):
        L["woff"].append(pe)
        pe += L["Np"][l] * L["Kp"][l]
        L["wtoff"].append(pe)
        pe += L["Np"][l] * L["Kp"][l]
    L["pack_elems"] = pe
    L["m_off"] = _r(L["params_floats"] * 4, 256)
    L["v_off"] = _r(L["m_off"] + L["trained_floats"] * 4, 256)
    L["pack_off"] = _r(L["v_off"] + L["trained_floats"] * 4, 256)
    L["bytes"] = _r(L["pack_off"] + pe * 2, 256)
    return L


def work_layout(F, power, mem, n_rot, n_ph, B):
    """The grad stage's workspace (float offsets), in the order of antsrl_memtrain_work_layout: the target's nine
    outputs, the model's nine, dh1 dh2 dh3 dg dr1 dr2 dqr dp1 dqp, the row-chunk partials, the loss partials; every
    block rounded up to 64 floats."""
    L = state_layout(F, power, mem, n_rot, n_ph)
    Bp = _r(B, 32)
    nch = min(64, (Bp + 255) // 256)
    chunk = _r((Bp + nch - 1) // nch, 32)
    W = dict(L=L, B=B, Bp=Bp, chunk=chunk, nchunk=(Bp + chunk - 1) // chunk, act=[[], []], dout=[], part_layer=[])
    off = 0

    def take(floats):
        nonlocal off
        o = off
        off = _r(off + floats, 64)
        return o
    for n in range(2):
        for l in range(9):
            W["act"][n].append(take(Bp * L["Np"][l]))
    for l in DOUT_ORDER:
        W["dout"].append(take(Bp * L["Np"][l]))
    pc = 0
    for l in range(9):
        W["part_layer"].append(pc)
        pc += L["Np"][l] * L["Kp"][l] + L["Np"][l]
    W["part_chunk"] = pc
    W["part"] = take(pc * W["nchunk"])
    W["nloss"] = (Bp + 255) // 256
    W["lossp"] = take(W["nloss"])
    W["bytes"] = off * 4
    return W


def read_workspace(work, W):
    """The workspace (a float32 CPU tensor over the device's bytes) as the image stage_outputs reads and writes."""
    L, Bp = W["L"], W["Bp"]
    img = {}
    for n in range(2):
        for l in range(9):
            img[("act", n, l)] = work[W["act"][n][l]: W["act"][n][l] + Bp * L["Np"][l]].view(Bp, L["Np"][l])
    for l in range(9):
        img[("dout", l)] = work[W["dout"][l]: W["dout"][l] + Bp * L["Np"][l]].view(Bp, L["Np"][l])
    img["part"] = work[W["part"]: W["part"] + W["nchunk"] * W["part_chunk"]].view(W["nchunk"], W["part_chunk"])
    img["lossp"] = work[W["lossp"]: W["lossp"] + W["nloss"]]
    return img


def read_packs(state_bytes, L):
    """The bf16 packs of a state buffer (a uint8 CPU tensor): [(W [Np][Kp], W^T [Kp][Np])] per trained layer, as float32."""
    pk = state_bytes[L["pack_off"]: L["pack_off"] + 2 * L["pack_elems"]].view(torch.bfloat16).float()
    return [(pk[L["woff"][l]: L["woff"][l] + L["Np"][l] * L["Kp"][l]].view(L["Np"][l], L["Kp"][l]),
             pk[L["wtoff"][l]: L["wtoff"][l] + L["Np"][l] * L["Kp"][l]].view(L["Kp"][l], L["Np"][l])) for l in range(9)]


def expected_packs(weights, L):
    """What the packs must hold for the nine master weights: bf16(W) and its transpose, zero padded."""
    out = []
    for l in range(9):
        w = torch.zeros((L["Np"][l], L["Kp"][l]))
        w[:L["out"][l], :L["inn"][l]] = weights[l].float().to(torch.bfloat16).float()
        out.append((w, w.T.contiguous()))
    return out


# ======================================================================================================================
# One launch at a time
# ======================================================================================================================
def problem(sd, target_sd, arrays, idx, B, discount, dims, stale=None):
    """What every stage reads beside the workspace: the nets' fp32 masters, the gathered x of both nets (zero rows up
    to Bp), the gathered actions / rewards / dones.  dims = (F, power, mem, n_rot, n_ph).  All CPU."""
    F, power, mem, n_rot, n_ph = dims
    W = work_layout(F, power, mem, n_rot, n_ph, B)
    st, ast, act, rw, nst, nast, dn = (t.cpu() for t in arrays)
    rows = torch.arange(B) if idx is None else idx.cpu()
    xs = []
    for s, a in ((nst, nast), (st, ast)):
        x = torch.zeros((W["Bp"], F + 2 + mem))
        x[:B] = _x(s[rows], a[rows])
        xs.append(x)
    nets = [dict(W=[d[l + ".weight"].detach().cpu().float() for l in TRAINED], b=[d[l + ".bias"].detach().cpu().float() for l in TRAINED])
            for d in (target_sd, sd)]
    return dict(W=W, L=W["L"], B=B, xs=xs, nets=nets, act=act[rows], rw=rw[rows].float(), dn=dn[rows].bool(),
                discount=_f32(discount), n=(n_rot, n_ph), stale=stale)


def _bf(t):
    return t.float().to(torch.bfloat16).float()


def _mm(a, wt, dt):
    """[R, K] x [K, N]: bf16 operands, products exact; float64: one sum; float32: 64-term blocks summed exactly, the
    blocks accumulated in fp32 in order (an order of its own, neither the MFMA's nor float64's)."""
    a, wt = _bf(a).double(), _bf(wt).double()
    if dt == torch.float64:
        return a @ wt
    acc = torch.zeros((a.shape[0], wt.shape[1]), dtype=torch.float32)
    for k in range(0, a.shape[1], 64):
        acc = acc + (a[:, k:k + 64] @ wt[k:k + 64]).float()
    return acc


def _mag(a, wt):
    return _bf(a).double().abs() @ _bf(wt).double().abs()


def _bound(K, mag):
    return gamma(K + 3) * mag + TINY * (K + 3) * (mag > 0)


def _forward(l, n, img, P, dt, defect):
    L, net = P["L"], P["nets"][n]
    out, inn, Np, Bp = L["out"][l], L["inn"][l], L["Np"][l], P["W"]["Bp"]
    w = P["stale"][n][l] if defect == "stale_pack" else net["W"][l]
    a = P["xs"][n] if IN_OF[l] < 0 else img[("act", n, IN_OF[l])][:, :inn]
    if defect == "last_column_dropped":
        a = a.clone()
        a[:, inn - 1] = 0.0
    z = _mm(a, w.T, dt) + net["b"][l].to(dt)
    if l == 3 and defect != "residual_dropped":
        z = z + P["xs"][n].to(dt)
    if l < 3:
        z = torch.relu(z)
    full = torch.zeros((Bp, Np), dtype=dt)
    full[:, :out] = z
    if defect == "bias_on_padding" and Np > out:  # the j < nb guard gone: the floats behind the bias, here the bias again
        pad = net["b"][l][torch.arange(out, Np) % out].to(dt)
        full[:, out:] = torch.relu(pad) if l < 3 else pad
    bnd = None
    if dt == torch.float64:
        mag = _mag(a, w.T) + net["b"][l].double().abs() + (P["xs"][n].double().abs() if l == 3 else 0.0)
        bnd = torch.zeros((Bp, Np), dtype=dt)
        bnd[:, :out] = _bound(inn, mag)
    return full, bnd


def _td(img, P, dt, defect):
    B, Bp, W = P["B"], P["W"]["Bp"], P["W"]
    rw = P["rw"].to(dt)
    nd = torch.ones((B,), dtype=dt) if defect == "dones_ignored" else torch.where(P["dn"], 0.0, 1.0).to(dt)
    outs, bnds = {}, {}
    contrib, pert = torch.zeros((Bp,), dtype=dt), torch.zeros((Bp,), dtype=torch.float64)
    for key, tkey, col, n in ((6, 6, 0, P["n"][0]), (8, 8, 1, P["n"][1])):
        q, qt = img[("act", 1, key)][:B, :n].to(dt), img[("act", 0, tkey)][:B, :n].to(dt)
        a = P["act"][:, col]
        ok = (a >= 0) & (a < n)
        norm = _f32(2.0 / B if defect == "scale_2_over_B" else 2.0 / (B * n))
        inv = _f32(1.0 / (B * n))
        boot = (P["discount"] * qt.max(dim=1).values) * nd
        qa = q.gather(1, a.clamp(0, n - 1).view(-1, 1)).view(-1)
        d = torch.where(ok, qa - (rw + boot), torch.zeros_like(rw))
        dq = torch.zeros((Bp, 32), dtype=dt)
        r = ok.nonzero().view(-1)
        dq[r, a[r]] = d[r] * norm
        outs[("dout", key)] = dq
        contrib[:B] += d * d * inv
        if dt == torch.float64:
            mag = torch.where(ok, qa.abs() + rw.abs() + boot.abs(), torch.zeros_like(rw))
            b = torch.zeros((Bp, 32), dtype=dt)
            b[r, a[r]] = _bound(3, mag[r] * norm)
            bnds[("dout", key)] = b
            e = gamma(3) * mag  # what the device's d may be off by
            pert[:B] += (2 * d.abs() * e + e * e) * inv
    nloss = W["nloss"]
    pad = torch.zeros((nloss * 256,), dtype=dt)
    pad[:Bp] = contrib
    if dt == torch.float64:
        outs["lossp"] = pad.view(nloss, 256).sum(1)
        pp = torch.zeros((nloss * 256,), dtype=dt)
        pp[:Bp] = pert
        pp = pp.view(nloss, 256).sum(1)
        bnds["lossp"] = gamma(256 + 3) * (outs["lossp"] + pp) + pp
        bnds["lossp"] = bnds["lossp"] + TINY * 259 * (bnds["lossp"] > 0)
    else:  # rows in order, not the kernel's tree
        s = torch.zeros((nloss,), dtype=dt)
        v = pad.view(nloss, 256)
        for j in range(256):
            s = s + v[:, j]
        outs["lossp"] = s
    return outs, bnds


def _backward(l, img, P, dt, defect):
    """dOut of layer l (and of layer 7 with it, for l = 4) -> dOut of its input layer."""
    L = P["L"]
    il = IN_OF[l]
    Bp, Npi, outi = P["W"]["Bp"], L["Np"][il], L["out"][il]
    segs = [l] if (l != 4 or defect == "dg_second_segment_omitted") else [4, 7]
    z, mag, K = 0.0, 0.0, 0
    for s in segs:
        d, w = img[("dout", s)][:, :L["out"][s]], P["nets"][1]["W"][s]
        if defect == "stale_pack":
            w = P["stale"][1][s]
        if defect == "w_for_wt":  # the W pack read with W^T's leading dimension: B(k, j) = pack_W[j * Np + k]
            wp = torch.zeros((L["Np"][s], L["Kp"][s]))
            wp[:L["out"][s], :L["inn"][s]] = w
            w = wp.reshape(-1).view(L["Kp"][s], L["Np"][s]).T[:L["out"][s], :L["inn"][s]]
        z = z + _mm(d, w, dt)
        K += L["out"][s]
        if dt == torch.float64:
            mag = mag + _mag(d, w)
    mask = None
    if il < 3:
        src = img[("act", 1, il)][:, :outi]
        if defect == "mask_from_wrong_layer":
            other = img[("act", 1, (il + 1) % 3)]
            src = other[:, torch.arange(outi) % L["out"][(il + 1) % 3]]
        mask = (src >= 0) if defect == "mask_ge_0" else (src > 0)
        z = z * mask.to(dt)
    full = torch.zeros((Bp, Npi), dtype=dt)
    full[:, :outi] = z
    bnd = None
    if dt == torch.float64:
        bnd = torch.zeros((Bp, Npi), dtype=dt)
        bnd[:, :outi] = _bound(K, mag * mask.to(dt) if mask is not None else mag)
    return full, bnd


def _wgrad(img, P, dt, defect):
    W, L, B = P["W"], P["L"], P["B"]
    part = torch.zeros((W["nchunk"], W["part_chunk"]), dtype=dt)
    bnd = torch.zeros_like(part) if dt == torch.float64 else None
    for c in range(W["nchunk"]):
        b0, b1 = c * W["chunk"], min((c + 1) * W["chunk"], W["Bp"])
        real = max(0, min(b1, B) - b0)
        if defect == "tail_rows_dropped" and c == W["nchunk"] - 1:
            b1 = min(b1, B // 32 * 32)  # the rows of the last, partial 32-row tile
        for l in range(9):
            out, inn, Np, Kp = L["out"][l], L["inn"][l], L["Np"][l], L["Kp"][l]
            dy = img[("dout", l)][b0:b1, :out]
            xin = (P["xs"][1] if IN_OF[l] < 0 else img[("act", 1, IN_OF[l])])[b0:b1, :inn]
            o = W["part_layer"][l]
            wv = part[c, o: o + Np * Kp].view(Np, Kp)
            bv = part[c, o + Np * Kp: o + Np * Kp + Np]
            wv[:out, :inn] = _mm(dy.T, xin, dt)
            if dt == torch.float64:
                bv[:out] = dy.double().sum(0)
                bnd[c, o: o + Np * Kp].view(Np, Kp)[:out, :inn] = _bound(real, _mag(dy.T, xin))
                bnd[c, o + Np * Kp: o + Np * Kp + out] = _bound(real, dy.double().abs().sum(0))
            else:  # 32-row blocks summed exactly, accumulated in fp32
                s = torch.zeros((out,), dtype=dt)
                for r0 in range(0, b1 - b0, 32):
                    s = s + dy[r0:r0 + 32].double().sum(0).float()
                bv[:out] = s
                if defect == "db_first_tile_only":
                    bv[32:] = 0.0
    return part, bnd


def _finalize(img, P, dt):
    W, L = P["W"], P["L"]
    part, lossp = img["part"].to(dt), img["lossp"].to(dt)
    src = []
    for l in range(9):
        out, inn, Np, Kp = L["out"][l], L["inn"][l], L["Np"][l], L["Kp"][l]
        o = W["part_layer"][l]
        src.append((o + torch.arange(out).view(-1, 1) * Kp + torch.arange(inn).view(1, -1)).reshape(-1))
        src.append(o + Np * Kp + torch.arange(out))
    src = torch.cat(src)
    cols = part[:, src]
    if dt == torch.float64:
        g, loss = cols.sum(0), lossp.sum()
        return (g, loss), (_bound(W["nchunk"], cols.abs().sum(0)), _bound(W["nloss"], lossp.abs().sum()))
    g = torch.zeros((src.numel(),), dtype=dt)
    for c in range(W["nchunk"] - 1, -1, -1):  # descending: not the kernel's order
        g = g + cols[c]
    loss = torch.zeros((), dtype=dt)
    for i in range(W["nloss"] - 1, -1, -1):
        loss = loss + lossp[i]
    return (g, loss), None


def stage_outputs(stage, img, P, dt=torch.float64, defect=None):
    """What launch `stage` (STAGES) writes, computed from the image's own buffers: (outputs by key, bounds by key).
    float64: the stage's reference, operands rounded to bf16 where the contract says so, products exact, one sum, and
    per output element the a-priori bound  gamma(K + 3) (sum |a||w| + |bias| + |residual|) + 2^-126 (K + 3)  on any
    fp32 evaluation of it (K: the real term count; padding has bound 0).  float32: the CPU restatement in an order of
    its own, bounds None; `defect` plants one wrong thing in it."""
    outs, bnds = {}, {}
    if stage.startswith("fwd"):
        for l in FWD_LAUNCH[int(stage[3:])]:
            for n in range(2):
                outs[("act", n, l)], bnds[("act", n, l)] = _forward(l, n, img, P, dt, defect)
    elif stage == "td":
        outs, bnds = _td(img, P, dt, defect)
    elif stage.startswith("bwd"):
        for l in BWD_LAUNCH[int(stage[3:])]:
            outs[("dout", IN_OF[l])], bnds[("dout", IN_OF[l])] = _backward(l, img, P, dt, defect)
    elif stage == "wgrad":
        outs["part"], bnds["part"] = _wgrad(img, P, dt, defect)
    else:
        (outs["grads"], outs["loss"]), b = _finalize(img, P, dt)
        if b is not None:
            bnds["grads"], bnds["loss"] = b
    return outs, bnds


def simulate(P, defect=None):
    """All 16 launches in fp32 on the CPU, each from the buffers the launches before it wrote."""
    img = {}
    for s in STAGES:
        img.update(stage_outputs(s, img, P, torch.float32, defect)[0])
    return img


def share_of_bound(got, ref, bnd):
    """max |got - ref| / bound over the elements (0 / 0 = 0, an error over a zero bound = inf; NaN = inf)."""
    err = (torch.as_tensor(got).double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def check_stage(stage, img, P, got=None):
    """The worst share of the bound over what `stage` wrote in `got` (default: the image itself), against the float64
    stage on the image's inputs."""
    ref, bnd = stage_outputs(stage, img, P, torch.float64)
    got = img if got is None else got
    return max(share_of_bound(got[k], ref[k], bnd[k]) for k in ref)
