"""The explore agent on the device: ExploreTrainer against the device-contract restatement and the
reference's arithmetic (tests/explore_train_ref.py), ExploreAgent's acting and fused loop, standalone and in-loop, and the
hand-over of its layer1 to CollectAgent."""
import os
import sys

import numpy as np
import pytest

import explore_train_ref as X
from agent_harness import drive_loop, inloop_runs
from agent_harness import make_env as _env
from agent_harness import param_tolerance as _param_tolerance
from agent_harness import ptr as _p
from agent_harness import same_rings as _same_rings
from agent_harness import stream as _stream

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _trainer(state, F, discount=0.5, lr=1e-4):
    """An ExploreTrainer holding state's model and (different) target net."""
    from antsrl_amd.train import ExploreTrainer
    tr = ExploreTrainer(F, "cuda", discount=discount, lr=lr)
    tr.load_state_dict(state["sd"])
    for k, v in tr._views(tr.target).items():
        v.copy_(state["target"][k])
    return tr


def _cases():
    for F, B in X.SHAPES:
        yield "F%d_B%d" % (F, B)
    for name in X.VARIANTS:
        yield name


def _make(name):
    """(state, device arrays, device idx or None, discount, B, F, the gathered batch of the restatement)."""
    if name in X.VARIANTS:
        state, arrays, idx, discount, B = X.make_variant(name)
        F = 17
    else:
        F, B = (int(s[1:]) for s in name.split("_"))
        state, arrays, idx = X.make_case(F, B, 100 * F + B)
        discount = 0.5
    batch = X.gather_clamped(arrays, idx, B)
    dev = tuple(a.cuda().contiguous() for a in arrays)
    return state, dev, (None if idx is None else idx.cuda()), discount, B, F, batch


# ---- 1. the step against the contract, and equal bits
@pytest.mark.parametrize("name", list(_cases()))
def test_step_equals_the_contract_and_equal_inputs_give_equal_bits(name):
    import torch
    state, dev, idx, discount, B, F, batch = _make(name)
    loss_ref, g_ref = X.contract_train_step(state, batch, discount, update=False)
    bound = X.fp32_sum_bounds(state, batch, discount)  # from the restatement and the inputs alone
    tr = _trainer(state, F, discount)
    assert tr.launches(B) == 2
    target0 = tr.target.clone()
    tr.grads.fill_(SENTINEL)
    before = {k: v.cpu() for k, v in tr.state_dict().items()}
    loss = float(tr.step(dev, idx))
    gd = {k: v.cpu() for k, v in tr.grad_dict().items()}
    share = X.worst_share(gd, g_ref, bound)
    share_l = abs(loss - loss_ref) / bound["loss"] if loss != loss_ref else 0.0
    # Adam from the device's own gradient: the moments bit for bit (the first step from a zero Adam state)
    X.adam(state, gd, tr.lr, tr.betas, tr.eps)
    st, after = tr.adam_state(), tr.state_dict()
    worst_p = 0.0
    for k in X.NAMES:
        assert torch.equal(st["exp_avg"][k].cpu(), state["m"][k]) and torch.equal(st["exp_avg_sq"][k].cpu(), state["v"][k]), k
        err = (after[k].cpu() - state["sd"][k]).abs()
        worst_p = max(worst_p, float((err / _param_tolerance(state["sd"][k], before[k])).max()))
    print("\nMEASURED %-16s share of the fp32 sum bound: gradient %.3g, loss %.3g; parameters %.3g of their tolerance"
          % (name, share, share_l, worst_p))
    assert np.isfinite(loss) and share <= 1.0 and share_l <= 1.0 and worst_p <= 1.0
    assert not bool((tr.grads == SENTINEL).any())
    assert torch.equal(tr.target, target0)  # the target's block is only read
    # a second step (non-zero Adam state) on the same rows, then the twins
    loss2 = float(tr.step(dev, idx))
    state2 = X.new_state({k: v.cpu() for k, v in after.items()}, state["target"])
    loss2_ref, g2_ref = X.contract_train_step(state2, batch, discount, update=False)
    b2 = X.fp32_sum_bounds(state2, batch, discount)
    assert X.worst_share({k: v.cpu() for k, v in tr.grad_dict().items()}, g2_ref, b2) <= 1.0 and abs(loss2 - loss2_ref) <= b2["loss"]
    # grad() + apply(), step(keep_grads=False) and a rerun give the bits of step()
    state0, _, _, _, _, _, _ = _make(name)
    for mode in ("grad_apply", "no_grads", "rerun"):
        tw = _trainer(state0, F, discount)
        tw.grads.fill_(SENTINEL)
        losses = []
        for _ in range(2):
            if mode == "grad_apply":
                losses.append(float(tw.grad(dev, idx)))
                tw.apply()
            else:
                losses.append(float(tw.step(dev, idx, keep_grads=mode != "no_grads")))
        assert losses == [loss, loss2], mode
        assert torch.equal(tw.model, tr.model) and torch.equal(tw._adam, tr._adam) and torch.equal(tw.target, target0), mode
        if mode == "no_grads":
            assert bool((tw.grads == SENTINEL).all())
        else:
            assert torch.equal(tw.grads, tr.grads), mode


# ---- 2. against the reference's arithmetic, in fp32
def test_twenty_steps_against_the_references_arithmetic():
    import torch
    F, B = 294, 256
    state, arrays, _ = X.make_case(F, B, 77, N=2000)
    dev = tuple(a.cuda().contiguous() for a in arrays)
    tr = _trainer(state, F)
    g = torch.Generator().manual_seed(5)
    worst = worst_l = 0.0
    for s in range(20):
        idx = torch.randint(0, 2000, (B,), generator=g)
        batch = X.gather(arrays, idx)
        # each step is compared from the device's own weights: the bound is that of ONE step's bfloat16 roundings
        host = X.new_state({k: v.cpu() for k, v in tr.state_dict().items()}, {k: v.cpu() for k, v in tr.target_state_dict().items()})
        bd, fs = X.bf16_bounds(host, batch), X.fp32_sum_bounds(host, batch)
        loss_ref, g_ref = X.fp32_train_step(host, batch, update=False)
        loss = float(tr.train_on(dev, idx.cuda(), done=(s % 7 == 6)))
        both = {k: torch.as_tensor(bd[k]) + torch.as_tensor(fs[k]) for k in X.NAMES}
        worst = max(worst, X.worst_share({k: v.cpu() for k, v in tr.grad_dict().items()}, g_ref, both))
        worst_l = max(worst_l, abs(loss - loss_ref) / (bd["loss"] + fs["loss"]))
    print("\nMEASURED 20 steps at (294, 256) against torch fp32 autograd: worst share of the bf16 bound, gradient %.3g, loss %.3g"
          % (worst, worst_l))
    assert worst <= 1.0 and worst_l <= 1.0 and tr.syncs == 2 and tr.step_count == 20


# ---- 3. acting
def _agent(**kw):
    from antsrl_amd.agent import ExploreAgent
    return ExploreAgent(epsilon=0.5, learning_rate=1e-3, min_replay=500, replay_size=3000, seed=7, **kw)


def test_get_action_acts_with_the_target_net():
    import torch
    from antsrl_amd.agent import ExploreAgent
    from antsrl_amd.policy import LinearPolicy
    env = _env()
    ag = ExploreAgent(seed=3)
    ag.setup(env)
    assert ag.name == "explore_agent_pytorch" and (ag.epsilon, ag.discount, ag.learning_rate) == (0.1, 0.5, 1e-4)
    assert (ag.minibatch, ag.min_replay, ag.replay_size, ag.update_target_every) == (256, 1000, 50000, 1)
    env.observe()
    rot, ph = ag.get_action(env.obs, env.agent_state, False, env=env)
    assert ph is None and rot.dtype == torch.int8 and rot.shape == (4, 64)
    rot = rot.clone()
    ref = LinearPolicy(294, "cuda", with_pheromone_head=False)
    ref.load_state_dict(ag.trainer.target_state_dict())
    want, none = ref.act(env.obs, env.agent_state)
    assert none is None and torch.equal(rot, want) and len(set(rot.view(-1).tolist())) > 1
    # what it is: the model's block overwritten, no sync -> the same actions; after the sync, the model's
    v0 = ag.trainer.version
    ag.trainer.model.copy_(torch.randn_like(ag.trainer.model) * 0.1)
    again, _ = ag.get_action(env.obs, env.agent_state, False, env=env)
    assert torch.equal(again, rot) and ag.trainer.version == v0
    ag.trainer.sync_target()
    ref.load_state_dict(ag.trainer.state_dict())
    synced, _ = ag.get_action(env.obs, env.agent_state, False, env=env)
    assert torch.equal(synced, ref.act(env.obs, env.agent_state)[0]) and not torch.equal(synced, rot)
    assert ag.trainer.version == v0 + 1


# ---- 4. the loop
def test_the_loop_equals_the_loop_driven_entry_by_entry():
    import torch
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.train import ExploreTrainer
    steps, E, N = 30, 4, 64
    ag = _agent()
    r = drive_loop(ag, ExploreTrainer, 256, False, lambda tr: torch.equal(tr.target, tr.model), steps, E, N, max_time=12)
    tr, rm = r.trainer, r.ring
    assert len(rm) == min(3000, steps * E * N) and tr.step_count == steps - 1  # 256 rows after step 0: below min_replay
    assert r.synced_after_done and all(r.synced_after_done) and tr.syncs >= 1  # the run crosses one done
    for t, (x, y) in enumerate(zip(r.losses, r.host_losses)):
        assert (x == 0 and y == 0) or float(x) == float(y), "step %d" % t
    for t, ((r0,), (r1,)) in enumerate(zip(r.acts, r.host_acts)):
        assert torch.equal(r0, r1), "actions, step %d" % t
    _same_rings(ag.replay_memory, rm)
    assert bool((rm.actions[:len(rm), 1] == 1).all())  # a NULL pheromone is stored as 1
    assert set(rm.actions[:len(rm), 0].unique().tolist()) <= {0, 1, 2}
    assert torch.equal(ag.trainer.model, tr.model) and torch.equal(ag.trainer._adam, tr._adam) and torch.equal(ag.trainer.target, tr.target)
    assert torch.equal(r.env_a.obs, r.env_b.obs)
    # no pheromone action ever reached the environment: the activation is what initialize set
    got = torch.empty((E, N, 2), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().antsrl_read_state(r.env_a._h, cm.S_ACTIVATION, _p(got), _stream()))
    assert torch.equal(got, r.activation)


def test_inloop_equals_standalone():
    import torch
    steps = 30
    ra, rb = inloop_runs(_agent, False, steps, E=4, N=64, max_time=12)  # steps 0..8 stay below min_replay and do not train
    a, b, after_sync = ra.agent, rb.agent, rb.after_sync
    # every step is an in-loop hit except the very first (its observation was produced before the loop) and the first
    # after each sync, training or not
    assert a.inloop_hits == 0 and after_sync >= 1 and b.inloop_hits == steps - 1 - after_sync
    for (r0,), (r1,) in zip(ra.acts, rb.acts):
        assert torch.equal(r0, r1)
    for x, y in zip(ra.losses, rb.losses):
        assert (x == 0 and y == 0) or float(x) == float(y)
    _same_rings(a.replay_memory, b.replay_memory)
    ta, tb = a.trainer, b.trainer
    assert torch.equal(ta.model, tb.model) and torch.equal(ta.target, tb.target) and torch.equal(ta._adam, tb._adam)
    assert (ta.step_count, ta.syncs) == (tb.step_count, tb.syncs) and ta.step_count > 0 and ta.syncs >= 1
    assert torch.equal(ra.env.obs, rb.env.obs)
    assert bool((a.replay_memory.actions[:len(a.replay_memory), 1] == 1).all())


# ---- 5. the hand-over to stage 2
def test_save_load_and_the_hand_over_to_the_collect_agent(tmp_path):
    import torch
    from antsrl_amd.agent import CollectAgent, ExploreAgent
    env = _env()
    a, b = ExploreAgent(seed=1), ExploreAgent(seed=2)
    a.setup(env)
    b.setup(env)
    sd = a.trainer.state_dict()
    assert list(sd) == ["layer1.weight", "layer1.bias", "layer2.weight", "layer2.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(32, 296), (32,), (3, 32), (3,)]
    path = str(tmp_path / "explore.h5")
    a.save_model(path)
    assert list(torch.load(path)) == list(sd)
    assert not torch.equal(b.trainer.model, a.trainer.model)
    b.load_model(path)
    for t in (b.trainer.state_dict(), b.trainer.target_state_dict()):  # load_model sets the target net too
        for k, v in t.items():
            assert torch.equal(v, sd[k]), k
    b.trainer.load_state_dict({"explore_model." + k: v for k, v in sd.items()})  # CollectModel's prefix is accepted
    assert torch.equal(b.trainer.model, a.trainer.model)
    # stage 2: CollectAgent on that layer1 and layer2, its own layer3
    plain, ca = CollectAgent(seed=4, learning_rate=1e-3), CollectAgent(seed=4, learning_rate=1e-3)
    plain.setup(env)
    ca.setup(env, explore_model=path)
    got, own = ca.trainer.state_dict(), plain.trainer.state_dict()
    for k in sd:
        assert torch.equal(got["explore_model." + k], sd[k]), k
    for k in ("layer3.weight", "layer3.bias"):
        assert torch.equal(got[k], own[k]) and torch.equal(ca.trainer.target_state_dict()[k], own[k]), k
    assert ca.trainer.version == plain.trainer.version + 1
    env.observe()
    rot, ph = (t.clone() for t in ca.get_action(env.obs, env.agent_state, False, env=env))
    want, _ = a.get_action(env.obs, env.agent_state, False, env=env)  # the same layer1 and layer2: the same rotation
    assert torch.equal(rot, want) and ph is not None
    with pytest.raises(KeyError):
        ca.trainer.load_state_dict(sd)  # load_state_dict keeps requiring all six tensors
    arrays, idx = _random_replay(1000, 294, 3)
    for _ in range(10):
        ca.trainer.step(arrays, idx)
    after = ca.trainer.state_dict()
    assert torch.equal(after["explore_model.layer1.weight"], sd["layer1.weight"]) and torch.equal(after["explore_model.layer1.bias"], sd["layer1.bias"])
    assert not torch.equal(after["explore_model.layer2.weight"], sd["layer2.weight"])


def test_the_saved_file_loads_into_the_references_explore_model(tmp_path):
    """Needs the reference's sources beside the repository; skipped where they are absent."""
    import torch
    from antsrl_amd.agent import ExploreAgent
    here = os.path.dirname(os.path.abspath(__file__))
    ref_root = os.environ.get("ANTSRL_REFERENCE") or os.path.normpath(os.path.join(here, "..", "..", "reference"))
    if not os.path.isdir(os.path.join(ref_root, "agents")):
        pytest.skip("the reference's sources are not on this machine")
    sys.path.insert(0, ref_root)
    try:
        mod = pytest.importorskip("agents.explore_agent_pytorch")
    finally:
        sys.path.remove(ref_root)
    a = ExploreAgent(seed=1)
    a.setup(_env())
    path = str(tmp_path / "explore.h5")
    a.save_model(path)
    m = mod.ExploreModel((7, 7, 6), [2], 3)
    m.load_state_dict(torch.load(path))
    for k, v in a.trainer.state_dict().items():
        assert torch.equal(m.state_dict()[k], v.cpu()), k


def _random_replay(N, F, seed, B=256):
    _, arrays, idx = X.make_case(F, B, seed, N=N)
    import torch  # noqa: F401
    return tuple(a.cuda().contiguous() for a in arrays), idx.cuda()


# ---- 6. learning happens
def test_the_loss_falls_on_one_minibatch_and_layer1_moves():
    import torch
    from antsrl_amd.train import ExploreTrainer
    arrays, idx = _random_replay(2000, 294, 21)
    tr = ExploreTrainer(294, "cuda", lr=1e-3, seed=1)
    w1, t0 = tr.state_dict()["layer1.weight"], tr.target.clone()
    losses = [tr.step(arrays, idx, keep_grads=False).clone() for _ in range(200)]  # no sync: the target stays frozen
    first, last = float(losses[0]), float(losses[-1])
    moved = float((tr.state_dict()["layer1.weight"] - w1).abs().max())
    print("\nMEASURED loss on one minibatch, 200 steps at lr 1e-3: %.5f -> %.5f; layer1 moved by up to %.3g" % (first, last, moved))
    assert torch.equal(tr.target, t0) and last < first and moved > 0.0
