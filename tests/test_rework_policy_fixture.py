"""The rework agent's net pinned to the reference's own classes (tests/golden/contract/rework_net_ref.npz, written by
tests/golden/make_rework_golden.py from CollectAgentRework.get_action): the comparator `layered` reproduces what the
reference's target net returned, in fp32 and under .double(), and `collapse64`, the restatement of the device's
collapse, gives the float64 forward when it is applied in float64: that pins the layer order, the bias propagation and
the obs-then-agent-state concatenation.  CPU only; tests/test_gpu_rework_policy.py holds the kernels to these."""
import numpy as np
import pytest
import torch

from rework_policy_ref import LAYERS, MODELS, actions, collapse64, layered, load_model


def steps(rec):
    for t in range(rec["obs"].shape[0]):
        yield t, torch.from_numpy(rec["obs"][t]), torch.from_numpy(rec["agent_state"][t])


def recorded_q(rec, t):
    return np.concatenate([rec["q_rot"][t], rec["q_ph"][t]], axis=1)


@pytest.mark.parametrize("model", MODELS)
def test_layered_fp32_reproduces_the_recorded_q(model):
    sd, rec = load_model(model)
    assert list(rec["state_dict_keys"]) == [l + s for l in LAYERS for s in (".weight", ".bias")] == list(sd.keys())
    assert rec["obs"].shape[0] >= 3 and rec["obs"].shape[1:] == (64, 7, 7, 6)
    for t, obs, ast in steps(rec):
        err = np.abs(layered(sd, obs, ast, torch.float32).numpy().astype(np.float64) - recorded_q(rec, t)).max()
        assert err <= rec["e_ref"][t], (model, t, err, rec["e_ref"][t])


@pytest.mark.parametrize("model", MODELS)
def test_layered_float64_reproduces_q64(model):
    sd, rec = load_model(model)
    for t, obs, ast in steps(rec):
        q64 = rec["q64"][t]
        assert q64.dtype == np.float64
        err = np.abs(layered(sd, obs, ast, torch.float64).numpy() - q64) / np.abs(q64).max()
        assert err.max() <= 1e-12, (model, t, err.max())
        # and e_ref is the distance of the two recorded forwards
        assert np.abs(recorded_q(rec, t).astype(np.float64) - q64).max() == rec["e_ref"][t]


@pytest.mark.parametrize("model", MODELS)
def test_collapse64_applied_in_float64_is_q64(model):
    """In front of its one rounding to fp32 (2^-24 relative per element: more than 1e-9) the collapsed map IS the net."""
    sd, rec = load_model(model)
    wc, bc = collapse64(sd, rounded=False)
    assert wc.shape == (6, 296) and bc.shape == (6,) and wc.dtype == bc.dtype == torch.float64
    for t, obs, ast in steps(rec):
        x = torch.cat([obs.reshape(64, -1), ast.reshape(64, 2)], dim=1).double()
        q64 = torch.from_numpy(rec["q64"][t])
        err = ((x @ wc.T + bc) - q64).abs().max() / q64.abs().max()
        assert float(err) <= 1e-9, (model, t, float(err))
    w32, b32 = collapse64(sd)  # what the device must hold: the same values rounded once
    assert w32.dtype == b32.dtype == torch.float32
    assert torch.equal(w32, wc.to(torch.float32)) and torch.equal(b32, bc.to(torch.float32))


@pytest.mark.parametrize("model", MODELS)
def test_recorded_actions_are_the_argmax_of_the_recorded_q(model):
    _, rec = load_model(model)
    for t in range(rec["obs"].shape[0]):
        rot, ph = actions(torch.from_numpy(recorded_q(rec, t)), 3)
        assert np.array_equal(rot.numpy(), rec["rotation"][t]) and np.array_equal(ph.numpy(), rec["pheromone"][t]), (model, t)
    if model == "spread":  # every action of both heads on at least 5 % of the rows
        for a, lo in ((rec["rotation"], -1), (rec["pheromone"], 0)):
            assert np.bincount(a.reshape(-1) - lo, minlength=3).min() >= 0.05 * a.size


def test_shape_inference_from_state_dict():
    from antsrl_amd.policy import REWORK_LAYERS, rework_shape_from_state_dict
    sd, _ = load_model("init")
    assert REWORK_LAYERS == LAYERS
    assert rework_shape_from_state_dict(sd) == dict(n_features=294, agent_dim=2, g1=64, g2=128, g3=32, r1=64, r2=128, r3=32,
                                                    p1=32, n_rot=3, n_ph=3)
    bad = dict(sd)
    bad["layer2.weight"] = torch.zeros(128, 65)
    with pytest.raises(AssertionError, match="layer2"):
        rework_shape_from_state_dict(bad)
