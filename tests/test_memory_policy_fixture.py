"""The memory agent net pinned to the reference's own classes (tests/golden/contract/memory_net_ref.npz, written by
tests/golden/make_memory_golden.py from CollectAgentMemory.get_action): the test comparator `fp32_forward` reproduces
the reference's q values and carried memory at every recorded step, and MemoryPolicy infers the net's shape from a
reference state_dict.  CPU only; tests/test_gpu_memory_policy.py holds the kernel to these comparators."""
import numpy as np
import pytest
import torch

from memory_policy_ref import MODELS, actions, bf16_forward, fp32_forward, load_model


@pytest.mark.parametrize("model", MODELS)
def test_fp32_comparator_reproduces_the_reference(model):
    sd, rec = load_model(model)
    assert list(rec["state_dict_keys"]) == list(sd.keys())  # the reference's names, in its order
    n = rec["obs"].shape[0]
    assert n >= 8
    for t in range(n):
        obs, ast, mem = (torch.from_numpy(rec[k][t]) for k in ("obs", "agent_state", "mem_in"))
        q_rot, q_ph, new = fp32_forward(sd, obs, ast, mem)
        for got, key in ((q_rot, "q_rot"), (q_ph, "q_ph"), (new, "mem_out")):
            want = rec[key][t]
            err = np.abs(got.numpy() - want) / np.maximum(1.0, np.abs(want))
            assert err.max() <= 1e-5, (model, t, key, float(err.max()))
        rot, ph = actions(q_rot, q_ph)
        assert np.array_equal(rot.numpy(), rec["a_rot"][t]) and np.array_equal(ph.numpy(), rec["a_ph"][t]), (model, t)
        if t + 1 < n:  # the memory is carried by the reference itself: step t's output is step t + 1's input
            assert np.array_equal(rec["mem_out"][t], rec["mem_in"][t + 1])
    assert np.abs(rec["mem_out"][-1]).max() > 1e-3  # the memory does move


@pytest.mark.parametrize("model", MODELS)
def test_bf16_comparator_stays_close_to_fp32(model):
    sd, rec = load_model(model)
    for t in range(rec["obs"].shape[0]):
        args = [torch.from_numpy(rec[k][t]) for k in ("obs", "agent_state", "mem_in")]
        f, b = fp32_forward(sd, *args), bf16_forward(sd, *args)
        for x, y in zip(f, b):  # bf16 operands: ~2^-8 relative per rounding, on q values of O(100) for the checkpoint
            assert float(((x - y).abs() / x.abs().clamp(min=1.0)).max()) < 1e-2


@pytest.mark.parametrize("model,want", [("good_model", (4, 10)), ("seeded_p5", (5, 20))])
def test_shape_inference_from_state_dict(model, want):
    from antsrl_amd.policy import memnet_shape_from_state_dict
    sd, _ = load_model(model)
    shp = memnet_shape_from_state_dict(sd)
    assert (shp["power"], shp["mem_size"]) == want
    assert shp["n_features"] == 294 and shp["n_rot"] == 3 and shp["n_ph"] == 3
