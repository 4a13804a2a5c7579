"""The seeded initial weights of the three policies: every seeded test net and the linear and explore trainers' initial
blocks are these draws, so the constructors must keep them bit for bit.  The restatement: ONE CPU generator seeded once;
per layer in state_dict order `rand(out, in)` then `rand(out)`, each mapped `(x * 2 - 1) / sqrt(in)` (nn.Linear's
default initialisation) as the constructors have always rounded it: the product with the Python float
`1.0 / math.sqrt(in)`.  A division by `math.sqrt(in)` differs from that in the last bit of some elements, and the bits
are what is pinned here."""
import math

import pytest
import torch

from antsrl_amd.policy import (LinearPolicy, MemoryPolicy, ReworkPolicy, memnet_param_shapes, rework_param_shapes)


def restated(shapes: dict, seed: int) -> dict:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    sd = {}
    for name, (out_f, in_f) in shapes.items():
        bound = 1.0 / math.sqrt(in_f)
        sd[name + ".weight"] = (torch.rand((out_f, in_f), generator=g) * 2 - 1) * bound
        sd[name + ".bias"] = (torch.rand((out_f,), generator=g) * 2 - 1) * bound
    return sd


def same(got: dict, want: dict) -> None:
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k


CASES = [(f, s) for f in (6, 294) for s in (0, 7)]


@pytest.mark.parametrize("n_features,seed", CASES)
@pytest.mark.parametrize("with_pheromone_head", [True, False])
def test_linear_policy_init(n_features, seed, with_pheromone_head):
    p = LinearPolicy(n_features, "cpu", with_pheromone_head=with_pheromone_head, seed=seed)
    shapes = dict(layer1=(32, n_features + 2), layer2=(3, 32))
    got = {"layer1.weight": p.w1, "layer1.bias": p.b1, "layer2.weight": p.w2, "layer2.bias": p.b2}
    if with_pheromone_head:
        shapes["layer3"] = (3, 32)
        got.update({"layer3.weight": p.w3, "layer3.bias": p.b3})
    else:
        assert p.w3 is None and p.b3 is None
    same(got, restated(shapes, seed))


@pytest.mark.parametrize("n_features,seed", CASES)
def test_memory_policy_init(n_features, seed):
    p = MemoryPolicy(n_features, "cpu", seed=seed)
    same(p.state_dict(), restated(memnet_param_shapes(n_features, 5, 20, 3, 3), seed))


@pytest.mark.parametrize("n_features,seed", CASES)
def test_rework_policy_init(n_features, seed):
    p = ReworkPolicy(n_features, "cpu", seed=seed)
    same(p.state_dict(), restated(rework_param_shapes(n_features), seed))
