"""Test comparators for the memory agent net (`CollectModelMemory`, agents/collect_agent_memory.py:24-78).  Test
infrastructure only.

`fp32_forward` restates the reference's forward in plain float32 PyTorch; tests/test_memory_policy_fixture.py pins it
to tests/golden/contract/memory_net_ref.npz, i.e. to what the reference's own classes returned.  `bf16_forward` is the
same net at the rounding points of the kernel's precision contract (antsrl_memnet.hip): bf16 weights and layer inputs,
fp32 accumulation, fp32 biases / ReLU / residual with the fp32 x / tanh / sigmoid / blend, memory carried in fp32.
"""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "memory_net_ref.npz")
LAYERS = ("layer1", "layer2", "layer3", "layer4", "rotation_layer1", "rotation_layer2", "rotation_layer3",
          "pheromone_layer1", "pheromone_layer2", "memory_layer1", "memory_layer2", "memory_layer3", "forget_layer")
MODELS = ("good_model", "seeded_p5")


def _x(obs, agent_state, memory):
    M = agent_state.reshape(-1, 2).shape[0]
    return torch.cat([obs.reshape(M, -1).to(torch.float32), agent_state.reshape(M, 2).to(torch.float32),
                      memory.reshape(M, -1).to(torch.float32)], dim=1)


def _forward(sd, obs, agent_state, memory, bf):
    dev = agent_state.device
    W = {k: v.to(dev, torch.float32) for k, v in sd.items()}

    def lin(name, t):
        return bf(t) @ bf(W[name + ".weight"]).T + W[name + ".bias"]

    x = _x(obs, agent_state, memory)
    old = memory.reshape(x.shape[0], -1).to(torch.float32)
    h = torch.relu(lin("layer1", x))
    h = torch.relu(lin("layer2", h))
    h = torch.relu(lin("layer3", h))
    g = lin("layer4", h) + x
    q_rot = lin("rotation_layer3", lin("rotation_layer2", lin("rotation_layer1", g)))
    q_ph = lin("pheromone_layer2", lin("pheromone_layer1", g))
    m = lin("memory_layer2", lin("memory_layer1", g))
    s = torch.sigmoid(lin("forget_layer", m))
    new = torch.tanh(lin("memory_layer3", m)) * s + old * (1 - s)
    return q_rot, q_ph, new


def fp32_forward(sd, obs, agent_state, memory):
    """(q_rot, q_ph, new_memory) in float32: CollectModelMemory.forward (collect_agent_memory.py:57-78)."""
    return _forward(sd, obs, agent_state, memory, lambda t: t)


def bf16_forward(sd, obs, agent_state, memory):
    """The same net at the kernel's rounding points (bf16 MFMA operands, everything else fp32)."""
    return _forward(sd, obs, agent_state, memory, lambda t: t.to(torch.bfloat16).to(torch.float32))


def actions(q_rot, q_ph):
    """rotation = argmax - n_rot // 2, pheromone = argmax (first maximum), collect_agent_memory.py:195-200."""
    return q_rot.argmax(dim=1) - q_rot.shape[1] // 2, q_ph.argmax(dim=1)


def top2_margin(q):
    t = q.topk(2, dim=1).values if q.shape[1] > 1 else torch.cat([q, q - float("inf")], dim=1)
    return t[:, 0] - t[:, 1]


def rebuild_seeded(rec, n_features=294, power=5, mem_size=20, n_rot=3, n_ph=3):
    """The seeded model's weights: nn.Linear in CollectModelMemory's construction order (collect_agent_memory.py:39-55)
    under torch.manual_seed(seed), checked against the fixture's per-tensor fingerprints."""
    from antsrl_amd.policy import memnet_param_shapes
    torch.manual_seed(int(rec["seed"]))
    sd = {}
    for name, (o, i) in memnet_param_shapes(n_features, power, mem_size, n_rot, n_ph).items():
        lin = torch.nn.Linear(i, o)
        sd[name + ".weight"], sd[name + ".bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    for k, v in sd.items():
        a = v.numpy().astype(np.float64)
        got = np.array([a.sum(), (a * a).sum(), a.reshape(-1)[0], a.reshape(-1)[-1]])
        assert np.allclose(got, rec["fp/" + k], rtol=1e-9, atol=1e-12), k
    return sd


def load_model(model):
    """-> (state_dict, recorded steps) of fixture model `model` (MODELS)."""
    z = np.load(FIXTURE)
    pre = model + "/"
    rec = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    if model == "seeded_p5":
        return rebuild_seeded(rec), rec
    return {n + s: torch.from_numpy(rec[n + s]) for n in LAYERS for s in (".weight", ".bias")}, rec
