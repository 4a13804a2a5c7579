"""Test comparators for the memory agent's training step (CollectAgentMemory.train, agents/collect_agent_memory.py:133-176).
Test infrastructure only.

`fp32_train_step` restates train() in plain float32 PyTorch with autograd; tests/test_memory_train_fixture.py pins it
to tests/golden/contract/memory_train_ref.npz, i.e. to what the reference's own agent computed.  `bf16_train_grads` is
the same gradient by manual backprop at the rounding points of the kernel's precision contract (antsrl_memtrain.hip):
bf16 MFMA operands (layer inputs, weights, dOut, saved activations), everything else fp32.  `adam_step` restates
torch.optim.Adam's single-tensor arithmetic as the apply stage performs it.
"""
import os

import numpy as np
import torch

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
    names = ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")
    return tuple(torch.from_numpy(np.ascontiguousarray(rec["rows/" + k][sel])) for k in names)


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
