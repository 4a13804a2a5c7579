"""The joint training step against the reference (tests/golden/contract/joint_train_ref.npz, recorded from the reference's
CollectAgent with requires_grad set again on its layer1 by tests/golden/make_joint_train_golden.py): fp32_train_step
reproduces the recorded losses, gradients and parameter changes of all six tensors to 1e-5 (the bound
test_linear_train_fixture.py uses for the same comparison), the fixture pins what the reference then trains (every
tensor, one shared ExploreModel, a target sync inside the call that sees done), and the device contract stands within
bfloat16's own error of the recording on every element of every call.  No GPU."""
import os

import numpy as np
import pytest
import torch

import joint_train_ref as J
from test_linear_train_fixture import batch_of

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "joint_train_ref.npz")
CALLS = 3


@pytest.fixture(scope="module")
def fx():
    return np.load(PATH)


def test_what_the_reference_trains_with_the_freeze_lifted(fx):
    assert list(fx["state_dict_keys"]) == list(J.NAMES)
    assert bool(fx["shared_explore"])                      # model and target net still share one ExploreModel
    assert fx["rows/agent_states"].shape[1:] == (2,)
    assert float(fx["discount"]) == 0.5 and float(fx["lr"]) == 1e-4
    for c in range(CALLS):
        assert len(fx["c%d/grad_none" % c]) == 0                                   # every tensor gets a gradient
        for k in J.NAMES:
            assert fx["c%d/delta/%s" % (c, k)].all()                              # and every float of it moves
    assert [int(fx["c%d/target_eq_model" % c]) for c in range(CALLS)] == [0, 1, 0]
    assert [bool(fx["c%d/done" % c]) for c in range(CALLS)] == [False, True, False]
    assert len(fx["c0/idx"]) == 264
    # the first Adam step moves every float by about lr
    for k in J.NAMES[:2]:
        assert np.allclose(np.abs(fx["c0/delta/" + k]), 1e-4, rtol=0.05)  # (lr g / (|g| + eps), and the rounding of after - before)
    # the same inputs as the linear recording: the same rows and the same initial weights
    lin = np.load(os.path.join(os.path.dirname(PATH), "linear_train_ref.npz"))
    for c in range(CALLS):
        assert np.array_equal(lin["c%d/idx" % c], fx["c%d/idx" % c])
    for k in J.NAMES:
        assert np.array_equal(lin["init/" + k], fx["init/" + k])


def test_fp32_train_step_reproduces_the_reference(fx):
    state = J.new_state({k: fx["init/" + k] for k in J.NAMES})
    worst = {}
    for c in range(CALLS):
        before = {k: v.clone() for k, v in state["sd"].items()}
        loss, grads = J.fp32_train_step(state, batch_of(fx, c))
        worst["loss"] = max(worst.get("loss", 0), abs(loss - float(fx["c%d/loss" % c])))
        assert abs(loss - float(fx["c%d/loss" % c])) <= 1e-5
        for k in J.NAMES:
            eg = float(np.abs(grads[k].numpy() - fx["c%d/grad/%s" % (c, k)]).max())
            ed = float(np.abs((state["sd"][k] - before[k]).numpy() - fx["c%d/delta/%s" % (c, k)]).max())
            worst["grad"], worst["delta"] = max(worst.get("grad", 0), eg), max(worst.get("delta", 0), ed)
            assert eg <= 1e-5 and ed <= 1e-5, (c, k, eg, ed)
        eq = all(torch.equal(state["sd"][k], t) for k, t in ((J.W3, state["target_w3"]), (J.B3, state["target_b3"])))
        if bool(fx["c%d/done" % c]):
            J.sync_target(state)
            eq = True
        assert eq == bool(fx["c%d/target_eq_model" % c])
    print("worst |error| against the fixture:", worst)


def test_contract_stands_within_bf16_of_the_recording(fx):
    """Every element of every gradient of every call, and the losses: the recording is the reference's fp32, the contract
    rounds x and w1 to bfloat16.  The bound is joint_train_ref.bf16_bounds from the fp32 state alone, with nothing added
    for the fp32 summation of either side."""
    state = J.new_state({k: fx["init/" + k] for k in J.NAMES})
    for c in range(CALLS):
        b = batch_of(fx, c)
        bd = J.bf16_bounds(state, b)
        lc, gc = J.contract_train_step(state, b, update=False)
        assert abs(lc - float(fx["c%d/loss" % c])) <= bd["loss"]
        ratio = 0.0
        for k in J.NAMES:
            err = (gc[k].double() - torch.as_tensor(fx["c%d/grad/%s" % (c, k)]).double()).abs()
            lim = bd[k]
            assert bool((err <= lim).all()), (c, k, float(err.max()), float(lim.max()))
            ratio = max(ratio, float(torch.where(err == 0, err, err / lim).max()))
        print("call %d: |loss_c - recorded| = %.3g (bound %.3g), worst gradient error / bound = %.3g"
              % (c, abs(lc - float(fx["c%d/loss" % c])), bd["loss"], ratio))
        J.fp32_train_step(state, b)  # the recording's own next weights
        if bool(fx["c%d/done" % c]):
            J.sync_target(state)
