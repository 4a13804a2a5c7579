"""PopulationMemoryAgent, P memory agents in lockstep (antsrl_amd/population.py; include/antsrl.h, "The population of
memory nets"; antsrl_popmemnet.hip) on the device.

1. The population equals its members: member p is, bit for bit, MemoryAgent's entries (MemoryTrainer, its acting policy
   with the carried memory, antsrl_agent_select, record_pre / _post with the memory, train_on) run alone on a shard
   handle of its Em environments with the member's own seed, epsilon, discount and learning rate: actions, explored
   flags, the new memory, rewards and loss after every step; the ring, both state blocks byte for byte, the acting pack,
   the gradients and the counters at the end.  The population's run goes under a sync debug mode that makes any
   read-back an error.  Both state_memory settings.  (population_harness.py holds the shapes and the comparison: its
   MEMORY kind.)
2. copy_member, with both memory halves.
3. save_model / load_model through the reference's 26 names.
4. driver.train_population.
(The stages alone: test_gpu_population_memory_agent_stages.py.)"""
import numpy as np
import pytest

from population_harness import MEMORY as H

pytestmark = pytest.mark.gpu

#: (a) is the harness's _A (P = 3, Em = 2, N = 20, bfloat16, epsilons (0, 0.5, 1), members 0 and 2 sharing a seed, K = None,
#: a 200-row ring that wraps in step 5, B = 48) with a small net; (b) is _B (P = 2, Em = 1, N = 32, float32, K = 24) with
#: the reference's B = 264, power 5 and mem 20.  max_time 8: an episode end and a target sync fall inside either run.
SHAPES, checked_run, make_envs, members_of = H.SHAPES, H.checked_run, H.make_envs, H.members_of


def test_the_shapes_are_the_issue_s():
    a, b = SHAPES["a"], SHAPES["b"]
    assert (a["P"], a["Em"], a["N"], a["bf16"], a["epsilon"], a["K"], a["B"], a["power"], a["mem"]) == (3, 2, 20, True, (0.0, 0.5, 1.0), None, 48, 4, 3)
    assert a["seed"][0] == a["seed"][2] != a["seed"][1] and a["Em"] * a["N"] * 5 >= a["ring"]
    assert (b["P"], b["Em"], b["N"], b["bf16"], b["K"], b["B"], b["power"], b["mem"]) == (2, 1, 32, False, 24, 264, 5, 20)
    assert a["max_time"] == b["max_time"] == 8


# ---- 1. the population equals its members
@pytest.mark.parametrize("name,state_memory", [("a", "reference"), ("a", "carried"), ("b", "reference")])
def test_the_population_equals_its_members(name, state_memory):
    import torch
    s = SHAPES[name]
    run = checked_run(name, state_memory)  # every comparison of the module docstring's point 1 is made in there
    end, P, Em = run.final, s["P"], s["Em"]
    explored = torch.stack([w.explored for w in run.log]).cpu().numpy().reshape(s["steps"], P, Em)
    for p in range(P):
        if s["epsilon"][p] == 0.0:
            assert not explored[:, p].any(), "member %d has epsilon 0 and explored" % p
        if s["epsilon"][p] == 1.0:
            assert explored[:, p].all(), "member %d has epsilon 1 and did not always explore" % p
    assert end.step_count >= 8 and end.syncs >= 1, (end.step_count, end.syncs)
    k = s["K"] or Em * s["N"]
    assert end.fill == s["ring"] and end.head == (k * s["steps"]) % s["ring"]  # the ring wrapped
    rot = torch.stack([w.rot for w in run.log]).view(s["steps"], P, -1)
    for p in range(P):
        for q in range(p + 1, P):
            assert not torch.equal(rot[:, p], rot[:, q]), (p, q)
            assert not torch.equal(end.model[p], end.model[q]), (p, q)
    losses = torch.stack([w.loss for w in run.log if torch.is_tensor(w.loss)])
    assert losses.shape == (end.step_count, P) and bool(torch.isfinite(losses).all())
    # the memory is carried: it leaves zero, and the rows of the ring hold it behind the agent state
    assert bool((run.log[-1].mem != 0).any()) and bool((end.agent_states[:, :, 2:] != 0).any())
    same = torch.equal(end.agent_states[:, :, 2:], end.new_agent_states[:, :, 2:])
    assert same == (state_memory == "reference"), "reference: the post-action memory in both; carried: the pre-action one in agent_states"
    if s["epsilon"][-1] == 1.0:  # a member that always explores gets its old memory back at every step: it stays zero
        Mm = Em * s["N"]
        assert not bool(run.log[-1].mem[(P - 1) * Mm:].any())


# ---- 2. copy_member
def test_copy_member():
    """Member 0 over member 2 on shape (a)'s population after its comparison: the state blocks (weights, Adam), the
    target, the acting pack, with `ring` the slab, and member 0's rows of BOTH memory halves; members 0 and 1 and the
    hyper-parameters stay; the population still steps."""
    import torch
    pop = checked_run("a").pop
    tr, Mm = pop.trainer, pop.g.Mm
    rows = lambda p: slice(p * Mm, (p + 1) * Mm)  # noqa: E731
    weights = lambda p: [t[p].clone() for t in (tr._model, tr._target, tr.packed)]  # noqa: E731
    memory = lambda p: [m[rows(p)].clone() for m in pop._mem]  # noqa: E731
    same = lambda xs, ys: all(torch.equal(a, b) for a, b in zip(xs, ys))  # noqa: E731
    # the memory halves of the members differ: member 2 always explored (zero), member 0 never did
    pop._mem[pop._cur][rows(2)].uniform_(-1, 1)
    assert not same(weights(0), weights(2)) and not same(memory(0), memory(2))
    # the harness's: the slabs differ; ring=False and ring=True; members 0 and 1; the epsilons; one more step
    H.check_copy_member(lambda p: weights(p) + memory(p), "weights, Adam, target, pack and memory are member 0's")


# ---- 3. files
def test_save_and_load_through_the_references_names(tmp_path):
    import torch
    from antsrl_amd.policy import MEMNET_LAYERS
    from antsrl_amd.population import PopulationMemoryAgent
    s = SHAPES["a"]
    env, _ = make_envs(s["P"], s["Em"], s["N"], 50, s["bf16"])
    pop = PopulationMemoryAgent(members_of(s), mem_size=s["mem"], power=s["power"], replay_size=100, minibatch=32, min_replay=64)
    pop.setup(env)
    tr = pop.trainer
    path = str(tmp_path / "member1.h5")
    pop.save_model(1, path)
    sd = torch.load(path, map_location="cpu")
    assert list(sd) == ["%s.%s" % (l, w) for l in MEMNET_LAYERS for w in ("weight", "bias")] and len(sd) == 26
    assert all(torch.equal(sd[k], v.cpu()) for k, v in tr.state_dict(1).items())
    pack1, pack2, adam0 = tr.packed[1].clone(), tr.packed[2].clone(), tr._model[0, tr._adam_range()].clone()
    assert not torch.equal(tr.packed[0], pack1)
    pop.load_model(path, 0)  # into member 0: model, target and acting pack; the others stay
    assert all(torch.equal(tr.state_dict(0)[k], sd[k].to(env.device)) for k in sd)
    assert all(torch.equal(tr.target_state_dict(0)[k], sd[k].to(env.device)) for k in sd)
    assert torch.equal(tr.packed[0], pack1) and torch.equal(tr.packed[1], pack1) and torch.equal(tr.packed[2], pack2)
    assert torch.equal(tr._model[0, tr._adam_range()], adam0), "Adam's state is kept"
    # setup(trained_model=) gives the file to every member
    pop2 = PopulationMemoryAgent(members_of(s), mem_size=s["mem"], power=s["power"], replay_size=100, minibatch=32, min_replay=64)
    pop2.setup(env, trained_model=path)
    for p in range(3):
        assert torch.equal(pop2.trainer.packed[p], pack1), p


# ---- 4. the driver
def test_train_population_drives_it():
    """P = 2, Em = 1, 32 ants, two episodes of 6 steps; 32 rows per step against min_replay = 64: it trains from the second
    step on.  Finite per-member logs of the right shape."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.driver import train_population
    from antsrl_amd.population import PopulationMemoryAgent
    P, N, EPISODES, STEPS = 2, 32, 2, 6
    env, _ = make_envs(P, 1, N, STEPS, False)
    members = [dict(epsilon=0.5, discount=0.5, learning_rate=1e-3, seed=7), dict(epsilon=0.9, discount=0.99, learning_rate=1e-4, seed=9)]
    pop = PopulationMemoryAgent(members, mem_size=3, power=4, replay_size=300, minibatch=32, min_replay=64, seed=3)
    gen = cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)
    log = train_population(pop, env, gen, EPISODES, STEPS, seed=21, report_every=STEPS)
    assert pop.trainer.step_count == EPISODES * STEPS - 1 and pop.trainer.syncs >= 1
    assert log["member_loss"].shape == (EPISODES, P) and np.isfinite(log["member_loss"]).all(), log["member_loss"]
    assert log["member_total"].shape == (EPISODES, P) and np.isfinite(log["member_total"]).all()
    assert log["member_reward"].shape == (EPISODES, P) and log["epsilons"].shape == (EPISODES, P)
    assert list(log["epsilons"][0]) == [0.5, 0.9] and list(log["report_episode"]) == [0, 1]
    assert bool((pop.previous_memory != 0).any()) and bool(torch.isfinite(pop.previous_memory).all())
