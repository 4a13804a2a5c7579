"""PopulationReworkAgent, P rework agents in lockstep (antsrl_amd/population.py; include/antsrl.h, "The population of
rework agents"; antsrl_poprework.hip) on the device.

1. The population equals its members: member p is, bit for bit, ReworkAgent's entries (ReworkTrainer and its acting
   policy) run alone on a shard handle of its Em environments with the member's own seed, epsilon, discount and learning
   rate — actions, explored flags, rewards and loss after every step; the ring, the blocks, the collapsed buffers, both
   Adam moments, gradients, the dicts and the counters at the end (population_harness.py holds the two shapes and the
   comparison) — with `fused_select` on and off, and the two give the same log.
2. copy_member, the collapsed buffer included.
3. driver.train_population, which drives this population as it is; the files.
4. What a sync and what a training step change.
(The entries alone: test_gpu_population_rework_stages.py.)"""
import ctypes as C

import numpy as np
import pytest

from agent_harness import ptr, stream
from population_harness import _A, _B, F, RING, Kind, population_trainer, synthetic_ring

pytestmark = pytest.mark.gpu

#: (a) is the harness's _A: B = 48 (three whole passes of the batch kernel), bfloat16, epsilons (0, 0.5, 1), Mm = 40: a
#: pass of the acting kernel straddles two colonies.  (b) is _B with B = 136 (nine passes, the last with 8 valid rows),
#: float32, K = 24.
SHAPES = dict(a=_A, b=dict(_B, B=136))


class ReworkKind(Kind):
    """PopulationReworkAgent against ReworkTrainer.  The variant is the population's fused_select, "fused" or "unfused";
    the lone member acts the same way: ReworkPolicy.act_select, or act and antsrl_agent_select_actions behind it."""

    variant = "fused"

    def population_kw(self, s, variant):
        return dict(fused_select=variant == "fused")

    def lone_act(self, s, p, t, tr, env, st, explored, variant):
        import torch
        if variant != "fused":
            return super().lone_act(s, p, t, tr, env, st, explored, variant)
        Mm = s["Em"] * s["N"]
        rot, ph = (torch.zeros((Mm,), dtype=torch.int8, device=env.device) for _ in range(2))
        tr.policy.act_select(env.obs, env.agent_state, seed=s["seed"][p], step=t, env_id_base=p * s["Em"], n_envs=s["Em"],
                             n_ants=s["N"], epsilon=s["epsilon"][p], out=(rot, ph), explored=explored, env=env)
        return rot, ph, None, None, {}

    def same_extra(self, pop, p, tr, st):
        """The dict has the reference's 20 tensors; the acting weights changed as often as the lone trainer's."""
        assert len(pop.trainer.state_dict(p)) == 20 and pop.trainer.version == tr.version

    def final_of(self, pop):
        return dict(model=pop.trainer.model.clone(), collapsed=pop.trainer.collapsed.clone())


REWORK = ReworkKind("PopulationReworkAgent", "ReworkTrainer", True, "model", SHAPES,
                    lambda t, p, tr: (("model", t.model[p], tr.model), ("target", t.target[p], tr.target),
                                      ("collapsed", t.collapsed[p], tr.policy.collapsed),
                                      ("adam m", t._adam[0, p], tr._adam[0]), ("adam v", t._adam[1, p], tr._adam[1]),
                                      ("grads", t.grads[p], tr.grads)))
H = REWORK


def test_the_kind_is_the_issue_s():
    assert (H.population, H.single, H.pheromone, H.final) == ("PopulationReworkAgent", "ReworkTrainer", True, "model")
    assert SHAPES["a"] is _A and SHAPES["a"]["B"] == 48 and SHAPES["a"]["bf16"]
    assert SHAPES["b"] == dict(_B, B=136) and not SHAPES["b"]["bf16"] and SHAPES["b"]["K"] == 24


# ---- 1. the population equals its members
@pytest.mark.parametrize("variant", ["fused", "unfused"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_the_population_equals_its_members(name, variant):
    import torch
    s = H.SHAPES[name]
    run = H.checked_run(name, variant)  # every comparison of the module docstring's point 1 is made in there
    assert run.pop.fused_select == (variant == "fused")
    end, P, Em = run.final, s["P"], s["Em"]
    explored = torch.stack([w.explored for w in run.log]).cpu().numpy().reshape(s["steps"], P, Em)
    for p in range(P):
        if s["epsilon"][p] == 0.0:
            assert not explored[:, p].any(), "member %d has epsilon 0 and explored" % p
        if s["epsilon"][p] == 1.0:
            assert explored[:, p].all(), "member %d has epsilon 1 and did not always explore" % p
        if 0.0 < s["epsilon"][p] < 1.0 and Em > 1:
            assert (explored[:, p].any(axis=1) & ~explored[:, p].all(axis=1)).any(), "member %d never had a mixed step" % p
    assert end.step_count >= 8 and end.syncs >= 1, (end.step_count, end.syncs)
    k = s["K"] or Em * s["N"]
    assert end.fill == s["ring"] and end.head == (k * s["steps"]) % s["ring"]  # the ring wrapped
    rot = torch.stack([w.rot for w in run.log]).view(s["steps"], P, -1)
    for p in range(P):
        for q in range(p + 1, P):
            assert not torch.equal(rot[:, p], rot[:, q]), (p, q)
            assert not torch.equal(end.model[p], end.model[q]) and not torch.equal(end.collapsed[p], end.collapsed[q]), (p, q)
    losses = torch.stack([w.loss for w in run.log if torch.is_tensor(w.loss)])
    assert losses.shape == (end.step_count, P) and bool(torch.isfinite(losses).all())


@pytest.mark.parametrize("name", ["a", "b"])
def test_fused_and_unfused_give_the_same_log(name):
    import torch
    fused, unfused = H.checked_run(name, "fused"), H.checked_run(name, "unfused")
    assert len(fused.log) == len(unfused.log) == H.SHAPES[name]["steps"]
    for t, (a, b) in enumerate(zip(fused.log, unfused.log)):
        for what in ("rot", "ph", "explored", "reward"):
            assert torch.equal(getattr(a, what), getattr(b, what)), (what, t)
        assert torch.is_tensor(a.loss) == torch.is_tensor(b.loss) and (torch.equal(a.loss, b.loss) if torch.is_tensor(a.loss) else a.loss == b.loss), t
        assert (a.idx is None) == (b.idx is None) and (a.idx is None or torch.equal(a.idx, b.idx)), t
    for what in ("model", "collapsed"):
        assert torch.equal(getattr(fused.final, what), getattr(unfused.final, what)), what


# ---- 2. copy_member
def test_copy_member():
    import torch
    from antsrl_amd import _lib
    run = H.checked_run("a", "fused")
    pop, tr = run.pop, run.pop.trainer
    weights = lambda p: [t.clone() for t in (tr.model[p], tr.target[p], tr.collapsed[p], tr._adam[:, p])]  # noqa: E731
    before_w = [weights(p) for p in range(3)]
    assert not torch.equal(before_w[0][0], before_w[2][0]) and not torch.equal(before_w[0][2], before_w[2][2])
    H.check_copy_member(weights, "model, target, collapsed buffer and Adam are member 0's")  # the other assertions are the harness's
    # member 2 acts with member 0's net: after a copy, its actions are the single entry's on its rows with member 0's buffer
    pop.copy_member(0, 2, ring=False)
    assert torch.equal(tr.collapsed[2], tr.collapsed[0])
    env, Mm = run.env, pop.g.Mm
    rot, ph = pop.get_action(env.obs, env.agent_state, False)
    rot2, ph2 = (torch.full((Mm,), 99, dtype=torch.int8, device=env.device) for _ in range(2))
    obs2, ast2 = env.obs.reshape(-1, F)[2 * Mm:].contiguous(), env.agent_state.reshape(-1, 2)[2 * Mm:].contiguous()
    _lib.check(_lib.load().antsrl_policy_rework(C.byref(tr.shape), ptr(tr.collapsed[0]), ptr(obs2), 1, ptr(ast2), Mm, ptr(rot2), ptr(ph2),
                                                None, stream()), "policy_rework")
    assert torch.equal(rot.reshape(-1)[2 * Mm:], rot2) and torch.equal(ph.reshape(-1)[2 * Mm:], ph2)


# ---- 3. the driver and the files
def test_train_population(tmp_path):
    """P = 2, Em = 1, 32 ants, two episodes of 6 steps; 32 rows per step against min_replay = 64: the population trains
    from the second step of the first episode on, 5 + 6 steps."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.driver import train_population
    from antsrl_amd.policy import ReworkPolicy
    from antsrl_amd.population import PopulationReworkAgent
    P, N, EPISODES, STEPS = 2, 32, 2, 6
    env, _ = H.make_envs(P, 1, N, STEPS, False)
    members = [dict(epsilon=0.5, discount=0.5, learning_rate=1e-3, seed=7), dict(epsilon=0.9, discount=0.99, learning_rate=1e-4, seed=9)]
    pop = PopulationReworkAgent(members, seed=3, replay_size=300, minibatch=32, min_replay=64)
    gen = cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)
    log = train_population(pop, env, gen, EPISODES, STEPS, seed=21, report_every=STEPS, save_as=str(tmp_path / "member%d.pt"))
    assert log["member_loss"].shape == (EPISODES, P) and np.isfinite(log["member_loss"]).all(), log["member_loss"]
    assert log["member_total"].shape == (EPISODES, P)
    assert pop.trainer.step_count == EPISODES * STEPS - 1, pop.trainer.step_count
    assert pop.trainer.syncs >= 1 and pop.trainer.version == pop.trainer.syncs
    for p in range(P):
        sd = torch.load(str(tmp_path / ("member%d.pt" % p)), map_location="cpu")
        lone = ReworkPolicy(F, env.device)
        lone.load_state_dict(sd)
        mine = pop.trainer.state_dict(p)
        assert list(lone.state_dict()) == list(mine) and all(torch.equal(lone.params[k], mine[k]) for k in mine), p
    # the round trip per member: member 1's file into member 0 sets its model, its target and its collapsed buffer;
    # Adam's moments stay
    tr = pop.trainer
    adam, version = tr._adam.clone(), tr.version
    assert not torch.equal(tr.model[0], tr.model[1])
    pop.load_model(str(tmp_path / "member1.pt"), 0)
    assert torch.equal(tr.model[0], tr.model[1]) and torch.equal(tr.target[0], tr.model[1]) and tr.version == version + 1
    lone = ReworkPolicy(F, env.device)
    lone.load_state_dict(torch.load(str(tmp_path / "member1.pt"), map_location="cpu"))
    assert torch.equal(tr.collapsed[0], lone.collapsed) and torch.equal(tr._adam, adam)
    pop.save_model(0, str(tmp_path / "again.pt"))
    again, first = torch.load(str(tmp_path / "again.pt")), torch.load(str(tmp_path / "member1.pt"))
    assert list(again) == list(first) and all(torch.equal(again[k], first[k]) for k in first)


# ---- 4. what moves the acting weights
def test_a_sync_moves_the_acting_weights_and_a_step_does_not():
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    P, B = 2, 40
    tr = population_trainer("PopulationReworkTrainer", P, (7, 7, 6), dev, (7, 9), (0.5, 0.99), (1e-3, 1e-3))
    ring = synthetic_ring(P, 256, (7, 7, 6), dev, seed=4)
    g = torch.Generator(device="cpu")
    g.manual_seed(2)
    collapsed, target, model = tr.collapsed.clone(), tr.target.clone(), tr.model.clone()
    assert tr.version == 0 and torch.equal(target, model)
    tr.step(ring, torch.randint(0, 256, (P, B), generator=g).to(dev))
    assert tr.version == 0 and torch.equal(tr.collapsed, collapsed) and torch.equal(tr.target, target)
    assert not torch.equal(tr.model, model)
    tr.sync_target()
    assert (tr.version, tr.syncs) == (1, 1) and torch.equal(tr.target, tr.model)
    for p in range(P):
        assert not torch.equal(tr.collapsed[p], collapsed[p]), p
