"""The linear agent's training step against the reference (tests/golden/contract/linear_train_ref.npz, recorded from the
reference's CollectAgent by tests/golden/make_linear_train_golden.py): fp32_train_step reproduces the recorded losses,
gradients and parameter changes to 1e-5 (the bound test_memory_train_fixture.py uses for the same kind of comparison),
the fixture pins what the reference trains (layer1 never, a target sync inside the call that sees done), and the device
contract stands within bfloat16's own error of it.  No GPU."""
import os

import numpy as np
import pytest
import torch

import linear_train_ref as R

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "linear_train_ref.npz")
CALLS = 3


@pytest.fixture(scope="module")
def fx():
    return np.load(PATH)


def batch_of(fx, c):
    pos = np.searchsorted(fx["rows/index"], fx["c%d/idx" % c])
    assert np.array_equal(fx["rows/index"][pos], fx["c%d/idx" % c])
    return tuple(fx["rows/" + k][pos] for k in ("states", "agent_states", "actions", "rewards", "new_states",
                                                "new_agent_states", "dones"))


def test_what_the_reference_trains(fx):
    assert list(fx["state_dict_keys"]) == list(R.NAMES)
    assert bool(fx["shared_explore"])                      # model and target net share one ExploreModel
    assert fx["rows/agent_states"].shape[1:] == (2,)       # no memory in the rows
    assert float(fx["discount"]) == 0.5 and float(fx["lr"]) == 1e-4
    for c in range(CALLS):
        assert list(fx["c%d/grad_none" % c]) == list(R.NAMES[:2])                  # layer1 gets no gradient
        for k in R.NAMES[:2]:
            assert not fx["c%d/delta/%s" % (c, k)].any()                          # and never moves: exactly 0
        for k in R.TRAINED:
            assert fx["c%d/delta/%s" % (c, k)].any()
    assert [bool(fx["c%d/target_eq_model" % c]) for c in range(CALLS)] == [False, True, False]
    assert [bool(fx["c%d/done" % c]) for c in range(CALLS)] == [False, True, False]
    assert len(fx["c0/idx"]) == 264


def test_fp32_train_step_reproduces_the_reference(fx):
    state = R.new_state({k: fx["init/" + k] for k in R.NAMES})
    worst = {}
    for c in range(CALLS):
        before = {k: v.clone() for k, v in state["sd"].items()}
        loss, grads = R.fp32_train_step(state, batch_of(fx, c))
        worst["loss"] = max(worst.get("loss", 0), abs(loss - float(fx["c%d/loss" % c])))
        assert abs(loss - float(fx["c%d/loss" % c])) <= 1e-5
        for k in R.TRAINED:
            eg = float(np.abs(grads[k].numpy() - fx["c%d/grad/%s" % (c, k)]).max())
            ed = float(np.abs((state["sd"][k] - before[k]).numpy() - fx["c%d/delta/%s" % (c, k)]).max())
            worst["grad"], worst["delta"] = max(worst.get("grad", 0), eg), max(worst.get("delta", 0), ed)
            assert eg <= 1e-5 and ed <= 1e-5, (c, k, eg, ed)
        for k in R.NAMES[:2]:
            assert torch.equal(state["sd"][k], before[k])
        if bool(fx["c%d/done" % c]):
            R.sync_target(state)
    print("worst |error| against the fixture:", worst)


def test_contract_stands_within_bf16_of_fp32(fx):
    """The bound is linear_train_ref.bf16_bounds: x and w1 are each rounded once to bfloat16 (unit roundoff 2^-9), so every
    product of layer1 is off by at most (2^-8 + 2^-18) |x w|; that is carried through the heads, the TD target (max is
    1-Lipschitz), the loss and the gradient sums with the fp32 forward's own |d| and |h|.  A slack of 1e-6 absolute covers
    the fp32 summation orders."""
    state = R.new_state({k: fx["init/" + k] for k in R.NAMES})
    for c in range(CALLS):
        b = batch_of(fx, c)
        bound = R.bf16_bounds(state, b)
        st, ast = torch.as_tensor(b[0]).reshape(264, -1), torch.as_tensor(b[1])
        h32 = torch.cat([st, ast], 1) @ state["sd"][R.NAMES[0]].T + state["sd"][R.NAMES[1]]
        eh = (R.contract_hidden(state["sd"], st, ast) - h32).abs().double()
        assert bool((eh <= bound["h"] + 1e-6).all())
        lc, gc = R.contract_train_step(state, b, update=False)
        lf, gf = R.fp32_train_step(state, b, update=True)
        assert abs(lc - lf) <= bound[("loss", 0)] + bound[("loss", 1)] + 1e-6
        ratio = 0.0
        for k in R.TRAINED:
            err = (gc[k] - gf[k]).abs().double()
            assert bool((err <= bound[k] + 1e-6).all()), (c, k, float(err.max()), float(bound[k].max()))
            ratio = max(ratio, float((err / (bound[k] + 1e-6)).max()))
        print("call %d: |loss_c - loss_f| = %.3g (bound %.3g), worst gradient error / bound = %.3g"
              % (c, abs(lc - lf), bound[("loss", 0)] + bound[("loss", 1)], ratio))
        if bool(fx["c%d/done" % c]):
            R.sync_target(state)


def test_acting_steps_are_recorded(fx):
    """The fixture's get_action(training=False) steps: the fp32 target net reproduces the recorded actions."""
    w = {k: torch.as_tensor(fx["act/w/" + k]) for k in R.NAMES}
    for s in range(4):
        x = torch.cat([torch.as_tensor(fx["act/s%d/obs" % s]).reshape(64, -1), torch.as_tensor(fx["act/s%d/agent_state" % s])], 1)
        out = x @ w[R.NAMES[0]].T + w[R.NAMES[1]]
        qr, qp = out @ w[R.NAMES[2]].T + w[R.NAMES[3]], out @ w[R.NAMES[4]].T + w[R.NAMES[5]]
        assert np.array_equal((qr.argmax(1) - 1).numpy().astype(np.int8), fx["act/s%d/rotation" % s])
        assert np.array_equal(qp.argmax(1).numpy().astype(np.int8), fx["act/s%d/pheromone" % s])


def test_the_acting_bound_leaves_out_at_most_one_percent(fx):
    """linear_train_ref.acting_gap_safe on the recorded steps: the decisions whose fp32 top-two gap is inside the bfloat16
    bound are at most 1 % of them, and on all the others the contract's own bfloat16 forward takes the recorded action."""
    w = {k: torch.as_tensor(fx["act/w/" + k]).double() for k in R.NAMES}
    left_out = total = 0
    for s in range(4):
        obs, ast = torch.as_tensor(fx["act/s%d/obs" % s]).reshape(64, -1), torch.as_tensor(fx["act/s%d/agent_state" % s])
        x = torch.cat([obs, ast], 1).double()
        hc = R.bf16(R.contract_hidden({k: v.float() for k, v in w.items()}, obs, ast)).double()
        for head, want in ((0, fx["act/s%d/rotation" % s] + 1), (1, fx["act/s%d/pheromone" % s])):
            safe, arg = R.acting_gap_safe(w, x, head)
            assert np.array_equal(arg.numpy()[safe.numpy()], want[safe.numpy()])
            qc = hc @ R.bf16(w[R.NAMES[2 + 2 * head]]).double().T + w[R.NAMES[3 + 2 * head]]
            assert np.array_equal(qc.argmax(1).numpy()[safe.numpy()], want[safe.numpy()])
            left_out += int((~safe).sum())
            total += 64
    print("left out: %d of %d decisions (%.2f %%)" % (left_out, total, 100.0 * left_out / total))
    assert left_out <= 0.01 * total
