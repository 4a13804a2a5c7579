"""Test comparators for the rework agent's net (`CollectModelRework`, agents/collect_agent_rework.py:24-63).  Test
infrastructure only.

`layered` restates the module's ten layers in PyTorch, float32 or float64; tests/test_rework_policy_fixture.py pins it
to tests/golden/contract/rework_net_ref.npz, i.e. to what the reference's own classes returned.  `collapse64` restates
antsrl_rework_collapse (include/antsrl.h): the layers multiplied out in float64 in the device's order of sums, rounded
once to float32; the device's buffer must equal it in every bit.  `synthetic` is the input recipe for shapes that have
no fixture.
"""
import math
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "rework_net_ref.npz")
LAYERS = ("layer1", "layer2", "layer3", "layer4", "rotation_layer1", "rotation_layer2", "rotation_layer3",
          "rotation_layer4", "pheromone_layer1", "pheromone_layer2")
MODELS = ("init", "spread")
#: the layers below each head's last one, in the order the collapse pushes through them
ROT_CHAIN = ("rotation_layer3", "rotation_layer2", "rotation_layer1", "layer4", "layer3", "layer2", "layer1")
PH_CHAIN = ("pheromone_layer1", "layer4", "layer3", "layer2", "layer1")


def layered(sd, obs, agent_state, dtype=torch.float32):
    """q [M, n_rot + n_ph] (rotation head, then pheromone head): CollectModelRework.forward (:49-63) in `dtype`, on the
    CPU."""
    W = {k: torch.as_tensor(v).detach().cpu().to(dtype) for k, v in sd.items()}
    M = agent_state.reshape(-1, 2).shape[0]
    x = torch.cat([obs.detach().cpu().reshape(M, -1).to(dtype), agent_state.detach().cpu().reshape(M, 2).to(dtype)], dim=1)

    def lin(name, t):
        return torch.nn.functional.linear(t, W[name + ".weight"], W[name + ".bias"])

    g = lin("layer4", lin("layer3", lin("layer2", lin("layer1", x))))
    q_rot = lin("rotation_layer4", lin("rotation_layer3", lin("rotation_layer2", lin("rotation_layer1", g))))
    q_ph = lin("pheromone_layer2", lin("pheromone_layer1", g))
    return torch.cat([q_rot, q_ph], dim=1)


def collapse64(sd, rounded=True):
    """(Wc float32 [NQ, D], bc float32 [NQ]) as antsrl_rework_collapse computes them: each head's last layer pushed down
    through the layers below it in float64, every product rounded before it is added, the contracted index ascending
    from zero (the bias: from the bias so far); one rounding to float32 at the end.  rounded=False: the float64 values
    in front of that rounding."""
    P = {k: torch.as_tensor(v).detach().cpu().numpy().astype(np.float32).astype(np.float64) for k, v in sd.items()}

    def head(last, chain):
        v, bc = P[last + ".weight"].copy(), P[last + ".bias"].copy()
        for l in chain:
            W, b = P[l + ".weight"], P[l + ".bias"]
            assert W.shape[0] == v.shape[1], (l, W.shape, v.shape)
            acc = np.zeros((v.shape[0], W.shape[1]))
            for i in range(W.shape[0]):
                bc = bc + v[:, i] * b[i]
                acc = acc + v[:, i:i + 1] * W[i][None, :]
            v = acc
        return v, bc

    (vr, br), (vp, bp) = head("rotation_layer4", ROT_CHAIN), head("pheromone_layer2", PH_CHAIN)
    wc, bc = np.concatenate([vr, vp]), np.concatenate([br, bp])
    if rounded:
        wc, bc = wc.astype(np.float32), bc.astype(np.float32)
    return torch.from_numpy(wc), torch.from_numpy(bc)


def row_errors(sd, obs, agent_state):
    """(per row max |layered fp32 - layered float64|, the float64 q)."""
    q64 = layered(sd, obs, agent_state, torch.float64)
    return (layered(sd, obs, agent_state, torch.float32).double() - q64).abs().max(dim=1).values, q64


def e_ref(sd, obs, agent_state):
    """The reference's own fp32 error on these inputs: the max over elements of |layered fp32 - layered float64|."""
    return float(row_errors(sd, obs, agent_state)[0].max())


def actions(q, n_rot):
    """(rotation, pheromone) = (argmax - n_rot // 2, argmax), first maximum, of q [M, n_rot + n_ph] (:171-174)."""
    return q[:, :n_rot].argmax(dim=1) - n_rot // 2, q[:, n_rot:].argmax(dim=1)


def top2_gap(q, n_rot):
    """Per row the smaller of the two heads' gaps between the largest and the second largest q (a head of one output has
    no second: its gap is infinite)."""
    def gap(h):
        if h.shape[1] == 1:
            return torch.full((h.shape[0],), float("inf"), dtype=h.dtype)
        t = h.topk(2, dim=1).values
        return t[:, 0] - t[:, 1]
    return torch.minimum(gap(q[:, :n_rot]), gap(q[:, n_rot:]))


def param_shapes(F, n_rot, n_ph):
    D = F + 2
    return dict(layer1=(64, D), layer2=(128, 64), layer3=(32, 128), layer4=(D, 32), rotation_layer1=(64, D),
                rotation_layer2=(128, 64), rotation_layer3=(32, 128), rotation_layer4=(n_rot, 32), pheromone_layer1=(32, D),
                pheromone_layer2=(n_ph, 32))


def synthetic(F, n_rot, n_ph, M, seed):
    """-> (state_dict, obs float32 [M, F], agent_state float32 [M, 2]) on the CPU.  Weights: nn.Linear's default init
    under the seed, weights x 3, biases x 0.1 (the fixture's `spread`: the actions then vary over the rows).
    Observations: rand * 255 where a second rand < 0.15, else 0, rounded to bfloat16, so that both observation formats
    carry equal values.  Agent state: uniform [0, 1)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd = {}
    for name, (o, i) in param_shapes(F, n_rot, n_ph).items():
        b = 1.0 / math.sqrt(i)
        sd[name + ".weight"] = (torch.rand((o, i), generator=g) * 2 - 1) * b * 3.0
        sd[name + ".bias"] = (torch.rand((o,), generator=g) * 2 - 1) * b * 0.1
    val, pick = torch.rand((M, F), generator=g) * 255.0, torch.rand((M, F), generator=g) < 0.15
    obs = torch.where(pick, val, torch.zeros(())).to(torch.bfloat16).to(torch.float32)
    return sd, obs, torch.rand((M, 2), generator=g)


def load_model(model):
    """-> (state_dict, recorded steps) of fixture model `model` (MODELS); `spread` is rebuilt from the stored weights and
    the two stored factors, in float32 as the generator did."""
    z = np.load(FIXTURE)
    pre = model + "/"
    rec = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    rec["state_dict_keys"] = z["state_dict_keys"]
    sd = {n + s: torch.from_numpy(z["w/" + n + s]) for n in LAYERS for s in (".weight", ".bias")}
    if model == "spread":
        f = {".weight": torch.from_numpy(z["w_factor"]), ".bias": torch.from_numpy(z["b_factor"])}
        sd = {k: v * f[k[k.rindex("."):]] for k, v in sd.items()}
    return sd, rec
