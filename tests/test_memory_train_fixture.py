"""The training step's comparators pinned to the reference's own CollectAgentMemory.train
(tests/golden/contract/memory_train_ref.npz, written by tests/golden/make_memory_train_golden.py): `fp32_train_step`
reproduces the reference's loss and gradients over its three recorded calls, its Adam deltas and the target sync, and
the bf16 comparator stays close to it.  CPU only; tests/test_gpu_memory_train.py holds the kernels to these."""
import numpy as np
import torch

from memory_train_ref import (TRAINED_KEYS, adam_step, bf16_train_grads, cosine, fixture_batch, fp32_train_step,
                              load_fixture)

MEMORY_HEAD = ("memory_layer1", "memory_layer2", "memory_layer3", "forget_layer")


def _fp(a):
    a = a.double()
    return np.array([float(a.sum()), float((a * a).sum()), float(a.reshape(-1)[0]), float(a.reshape(-1)[-1])])


def _replay_reference():
    """Runs the fixture's three calls with fp32_train_step + torch.optim.Adam: yields (c, loss, grads, deltas, sd, target)."""
    sd, rec = load_fixture()
    discount, lr = float(rec["discount"]), float(rec["lr"])
    params = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=lr)  # the reference's optimizer over model.parameters()
    target = {k: v.clone() for k, v in sd.items()}
    counter = 0
    for c in range(3):
        cur = {k: p.detach().clone() for k, p in params.items()}
        loss, grads = fp32_train_step(cur, target, fixture_batch(rec, c), discount)
        opt.zero_grad()
        for k in TRAINED_KEYS:
            params[k].grad = grads[k].clone()
        opt.step()
        after = {k: p.detach().clone() for k, p in params.items()}
        if bool(rec["c%d/done" % c]):
            counter += 1
        if counter >= 1:
            target = {k: v.clone() for k, v in after.items()}
            counter = 0
        yield c, rec, loss, grads, {k: after[k] - cur[k] for k in after}, after, target


def test_fixture_shape():
    sd, rec = load_fixture()
    assert list(rec["state_dict_keys"]) == list(sd.keys())
    for c in range(3):
        assert rec["c%d/idx" % c].shape == (264,)
        assert sorted(rec["c%d/grad_none" % c]) == sorted(l + s for l in MEMORY_HEAD for s in (".weight", ".bias"))
    assert [bool(rec["c%d/target_eq_model" % c]) for c in range(3)] == [False, True, False]


def test_fp32_comparator_reproduces_the_reference():
    for c, rec, loss, grads, deltas, after, target in _replay_reference():
        pre = "c%d/" % c
        assert abs(float(loss) - float(rec[pre + "loss"])) <= 1e-5 * abs(float(rec[pre + "loss"])), (c, float(loss))
        for k in TRAINED_KEYS:
            g = grads[k]
            want_fp = rec[pre + "grad_fp/" + k]
            scale = float(np.sqrt(want_fp[1] / g.numel()))  # rms of the reference gradient
            got_s = g.reshape(-1)[torch.from_numpy(rec["sample/" + k])].double().numpy()
            err = np.abs(got_s - rec[pre + "grad_s/" + k]).max() / max(np.abs(rec[pre + "grad_s/" + k]).max(), scale)
            assert err <= 1e-5, (c, k, err)
            assert abs(_fp(g)[1] - want_fp[1]) <= 1e-5 * want_fp[1], (c, k)
        for k, d in deltas.items():
            want = rec[pre + "delta_s/" + k]
            got = d.reshape(-1)[torch.from_numpy(rec["sample/" + k])].double().numpy()
            if k.split(".")[0] in MEMORY_HEAD:  # never trained: exactly unchanged, in the reference and here
                assert not np.any(want) and not np.any(got) and not np.any(rec[pre + "delta_fp/" + k]), (c, k)
            else:  # Adam's first steps move by ~lr per element: agree to a small fraction of lr
                assert np.abs(got - want).max() <= 0.02 * float(rec["lr"]), (c, k, np.abs(got - want).max())
        eq = all(torch.equal(target[k], after[k]) for k in after)
        assert eq == bool(rec[pre + "target_eq_model"]), c


def test_bf16_comparator_stays_close_to_fp32():
    for c, rec, loss, grads, deltas, after, target in _replay_reference():
        cur = {k: after[k] - deltas[k] for k in after}
        pre_target = target if c != 1 else None
        if pre_target is None:  # call 1 synced after its step: its target was the initial weights
            pre_target, _ = load_fixture()
        bl, bg = bf16_train_grads(cur, pre_target, fixture_batch(rec, c), float(rec["discount"]))
        assert abs(float(bl) - float(loss)) <= 1e-2 * abs(float(loss)), (c, float(bl), float(loss))
        for k in TRAINED_KEYS:
            assert cosine(bg[k], grads[k]) >= 0.99, (c, k, cosine(bg[k], grads[k]))


def test_adam_restatement_matches_torch():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(1000, generator=g)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=1e-3, foreach=False)
    mine, m, v = p0.clone(), torch.zeros(1000), torch.zeros(1000)
    for s in range(1, 6):
        grad = torch.randn(1000, generator=g) * (torch.rand(1000, generator=g) > 0.2)
        p.grad = grad.clone()
        opt.step()
        mine, m, v = adam_step(mine, grad, m, v, s, 1e-3)
        ulp = (p.detach() - mine).abs().max() / torch.finfo(torch.float32).eps
        assert float(ulp) <= 8, (s, float(ulp))
