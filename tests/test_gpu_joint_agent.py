"""CollectAgent(train_layer1=True) on the device, the third stage of the linear agent's curriculum: its
fused loop against the same loop driven entry by entry, in-loop against standalone acting, the acting policy's live views
of the trainer's buffers, the hand-over from a frozen CollectAgent's file, and what save_model writes."""
import pytest

import joint_train_ref as J
from agent_harness import drive_loop, inloop_runs
from agent_harness import make_env as _env
from agent_harness import random_linear_replay as _random_replay
from agent_harness import same_rings as _same_rings

pytestmark = pytest.mark.gpu


def _agent(**kw):
    from antsrl_amd.agent import CollectAgent
    kw.setdefault("train_layer1", True)
    return CollectAgent(epsilon=0.5, learning_rate=1e-3, min_replay=500, replay_size=3000, seed=7, **kw)


def _same_trainers(ta, tb):
    import torch
    assert torch.equal(ta.model, tb.model) and torch.equal(ta.target_l3, tb.target_l3) and torch.equal(ta._adam, tb._adam)
    assert (ta.step_count, ta.syncs) == (tb.step_count, tb.syncs)


def test_the_argument_is_keyword_only_and_off_by_default():
    from antsrl_amd import JointTrainer
    from antsrl_amd.agent import CollectAgent
    from antsrl_amd.train import LinearTrainer
    import antsrl_amd
    assert "JointTrainer" in antsrl_amd.__all__ and JointTrainer.entry == "jointtrain" and JointTrainer.minibatch == 264
    with pytest.raises(TypeError):
        CollectAgent(0.1, 0.5, 3, 3, 1e-4, True)
    env = _env()
    a, b = CollectAgent(seed=3), CollectAgent(seed=3, train_layer1=True)
    a.setup(env)
    b.setup(env)
    assert type(a.trainer) is LinearTrainer and type(b.trainer) is JointTrainer and b.name == "collect_agent"
    assert (b.epsilon, b.discount, b.learning_rate, b.minibatch, b.min_replay) == (0.1, 0.5, 1e-4, 264, 1000)
    import torch
    for k, v in a.trainer.state_dict().items():  # the same seed gives the same net, frozen or not
        assert torch.equal(v, b.trainer.state_dict()[k]), k


def test_the_loop_equals_the_loop_driven_entry_by_entry_and_layer1_moves():
    import torch
    from antsrl_amd.train import JointTrainer
    steps, E, N = 36, 4, 64
    ag = _agent()
    r = drive_loop(ag, JointTrainer, 264, True, lambda tr: torch.equal(tr.target_l3, tr.model[tr._l3]), steps, E, N, max_time=12)
    tr, rm = r.trainer, r.ring
    assert type(ag.trainer) is JointTrainer
    assert len(rm) == min(3000, steps * E * N) and tr.step_count == steps - 1  # 256 rows after step 0: below min_replay
    assert r.synced_after_done and all(r.synced_after_done)
    for t, (x, y) in enumerate(zip(r.losses, r.host_losses)):
        assert (x == 0 and y == 0) or float(x) == float(y), "step %d" % t
    for t, ((r0, p0), (r1, p1)) in enumerate(zip(r.acts, r.host_acts)):
        assert torch.equal(r0, r1) and torch.equal(p0, p1), "actions, step %d" % t
    _same_rings(ag.replay_memory, rm)
    _same_trainers(ag.trainer, tr)
    assert torch.equal(r.env_a.obs, r.env_b.obs)
    # layer1 has moved; the same run with the freeze in place leaves it bit-identical to its start
    start = JointTrainer(294, "cuda", lr=1e-3, seed=7).state_dict()
    after = ag.trainer.state_dict()
    for k in J.NAMES[:2]:
        assert not torch.equal(after[k], start[k]), k
    frozen = _agent(train_layer1=False)
    env = _env(E, N, 12)
    frozen.setup(env)
    frozen.initialize(env)
    env.observe()
    frozen.run(env, steps)
    fsd = frozen.trainer.state_dict()
    assert frozen.trainer.step_count == steps - 1
    for k in J.NAMES[:2]:
        assert torch.equal(fsd[k], start[k]), k
    assert not torch.equal(fsd[J.W2], start[J.W2])


def test_layer1_moves_at_the_first_training_step():
    import torch
    ag = _agent()
    env = _env(4, 64, 12)
    ag.setup(env)
    ag.initialize(env)
    env.observe()
    start = ag.trainer.state_dict()
    losses = ag.run(env, 2)  # step 0 records 256 rows (below min_replay), step 1 trains
    assert losses[0] == 0 and float(losses[1]) > 0 and ag.trainer.step_count == 1
    after = ag.trainer.state_dict()
    for k in J.NAMES:
        assert not torch.equal(after[k], start[k]), k
    moved = (after[J.W1] - start[J.W1]).abs()
    assert float(moved.max()) <= 1.01e-3  # the first Adam step moves a float by at most lr


def test_inloop_equals_standalone():
    import torch
    a, b = inloop_runs(_agent, True, steps=36, E=4, N=64, max_time=12)  # steps 0..9 stay below min_replay and do not train
    assert b.agent.inloop_hits >= 8 and a.agent.inloop_hits == 0  # the steps below min_replay took the observation kernel's actions
    for (r0, p0), (r1, p1) in zip(a.acts, b.acts):
        assert torch.equal(r0, r1) and torch.equal(p0, p1)
    for x, y in zip(a.losses, b.losses):
        assert (x == 0 and y == 0) or float(x) == float(y)
    _same_rings(a.agent.replay_memory, b.agent.replay_memory)
    _same_trainers(a.agent.trainer, b.agent.trainer)
    assert torch.equal(a.env.obs, b.env.obs) and a.agent.trainer.step_count > 0


def test_the_acting_policy_is_live_views_of_the_trainer():
    import torch
    from antsrl_amd.policy import LinearPolicy
    from antsrl_amd.train import JointTrainer
    arrays, g = _random_replay(1000, 294, 3, True)
    idx = torch.randint(0, 1000, (264,), device="cuda", generator=g)
    tr = JointTrainer(294, "cuda", lr=1e-2, seed=5)
    env = _env()
    env.observe()
    first = tuple(t.clone() for t in tr.policy.act(env.obs, env.agent_state))
    for s in range(5):
        v = tr.version
        tr.train_on(arrays, idx, done=(s == 2))
        assert tr.version == v + (2 if s == 2 else 1)  # the step, and the sync
        fresh = LinearPolicy(294, "cuda")
        fresh.load_state_dict(tr.target_state_dict())
        got, want = tr.policy.act(env.obs, env.agent_state), fresh.act(env.obs, env.agent_state)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), s
    p = tr.policy
    assert p.w1.data_ptr() == tr.model.data_ptr() and p.w3.data_ptr() == tr.target_l3.data_ptr()
    assert tr.syncs == 1 and not torch.equal(p.w3, tr.state_dict()[J.W3])  # two steps behind the sync: the target's layer3 acts
    last = tr.policy.act(env.obs, env.agent_state)
    assert not (torch.equal(first[0], last[0]) and torch.equal(first[1], last[1]))  # five steps at lr 1e-2 change decisions


def test_hand_over_from_a_frozen_agents_file_and_save_model(tmp_path):
    import torch
    from antsrl_amd.agent import CollectAgent
    env = _env()
    frozen = CollectAgent(seed=11, learning_rate=1e-3)
    frozen.setup(env)
    arrays, g = _random_replay(1000, 294, 4, True)
    idx = torch.randint(0, 1000, (264,), device="cuda", generator=g)
    for _ in range(3):
        frozen.trainer.step(arrays, idx)  # layer3 now differs from its target copy: the file holds the model's
    path = str(tmp_path / "collect.h5")
    frozen.save_model(path)
    sd = frozen.trainer.state_dict()
    joint = CollectAgent(seed=12, learning_rate=1e-3, train_layer1=True)
    joint.setup(env, trained_model=path)
    tr = joint.trainer
    for d in (tr.state_dict(), tr.target_state_dict()):  # load_model sets the target net too
        assert list(d) == list(J.NAMES)
        for k in J.NAMES:
            assert torch.equal(d[k], sd[k]), k
    assert tr.step_count == 0 and not bool(tr._adam.any())
    # the first joint step starts from exactly those six tensors: its gradient is the contract's on them
    batch = tuple(a[idx].cpu().numpy() for a in arrays)
    host = J.new_state({k: v.cpu() for k, v in sd.items()})
    loss_ref, g_ref = J.contract_train_step(host, batch, update=False)
    bound = J.fp32_sum_bounds(host, batch)
    loss = float(tr.step(arrays, idx))
    assert J.worst_share({k: v.cpu() for k, v in tr.grad_dict().items()}, g_ref, bound) <= 1.0
    assert abs(loss - loss_ref) <= bound["loss"]
    # save_model: six tensors under CollectModel's names, on the CPU, and the round trip
    out = str(tmp_path / "joint.h5")
    joint.save_model(out)
    saved = torch.load(out)
    assert list(saved) == list(J.NAMES)
    assert [tuple(v.shape) for v in saved.values()] == [(32, 296), (32,), (3, 32), (3,), (3, 32), (3,)]
    for k, v in tr.state_dict().items():
        assert saved[k].device.type == "cpu" and torch.equal(saved[k], v.cpu()), k
    assert not torch.equal(saved[J.W1], sd[J.W1].cpu())
    frozen.load_model(out)  # and a frozen agent takes the file back
    for k, v in frozen.trainer.state_dict().items():
        assert torch.equal(v.cpu(), saved[k]), k
    # explore_model= goes under the joint trainer's heads as under the frozen one's
    other = CollectAgent(seed=13, train_layer1=True)
    four = {k[len("explore_model."):]: v for k, v in saved.items() if k.startswith("explore_model.")}
    four_path = str(tmp_path / "explore.h5")
    torch.save(four, four_path)
    own = CollectAgent(seed=13, train_layer1=True)
    own.setup(env)
    other.setup(env, explore_model=four_path)
    got = other.trainer.state_dict()
    for k in J.NAMES[:4]:
        assert torch.equal(got[k].cpu(), saved[k]), k
    for k in J.NAMES[4:]:
        assert torch.equal(got[k], own.trainer.state_dict()[k]) and torch.equal(other.trainer.target_state_dict()[k], got[k]), k
