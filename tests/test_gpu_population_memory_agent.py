"""PopulationMemoryAgent, P memory agents in lockstep (antsrl_amd/population.py; include/antsrl.h, "The population of
memory nets"; antsrl_popmemnet.hip) on the device.

1. The population equals its members: member p is, bit for bit, MemoryAgent's entries (MemoryTrainer, its acting policy
   with the carried memory, antsrl_agent_select, record_pre / _post with the memory, train_on) run alone on a shard
   handle of its Em environments with the member's own seed, epsilon, discount and learning rate: actions, explored
   flags, the new memory, rewards and loss after every step; the ring, both state blocks byte for byte, the acting pack,
   the gradients and the counters at the end.  The population's run goes under a sync debug mode that makes any
   read-back an error.  Both state_memory settings.
2. copy_member, with both memory halves.
3. save_model / load_model through the reference's 26 names.
4. driver.train_population.
(The stages alone: test_gpu_population_memory_agent_stages.py.)"""
from types import SimpleNamespace

import numpy as np
import pytest

from agent_harness import ptr, same_rings, stream
from population_harness import _A, _B, RING, make_envs, members_of

pytestmark = pytest.mark.gpu

F = 294
#: (a) is the harness's _A (P = 3, Em = 2, N = 20, bfloat16, epsilons (0, 0.5, 1), members 0 and 2 sharing a seed, K = None,
#: a 200-row ring that wraps in step 5, B = 48) with a small net; (b) is _B (P = 2, Em = 1, N = 32, float32, K = 24) with
#: the reference's B = 264, power 5 and mem 20.  max_time 8: an episode end and a target sync fall inside either run.
SHAPES = dict(a=dict(_A, power=4, mem=3), b=dict(_B, B=264, power=5, mem=20))
_RUNS = {}


def test_the_shapes_are_the_issue_s():
    a, b = SHAPES["a"], SHAPES["b"]
    assert (a["P"], a["Em"], a["N"], a["bf16"], a["epsilon"], a["K"], a["B"], a["power"], a["mem"]) == (3, 2, 20, True, (0.0, 0.5, 1.0), None, 48, 4, 3)
    assert a["seed"][0] == a["seed"][2] != a["seed"][1] and a["Em"] * a["N"] * 5 >= a["ring"]
    assert (b["P"], b["Em"], b["N"], b["bf16"], b["K"], b["B"], b["power"], b["mem"]) == (2, 1, 32, False, 24, 264, 5, 20)
    assert a["max_time"] == b["max_time"] == 8


def run_population(s, state_memory):
    """The population's `steps` rollout_steps with any read-back an error; per step (device copies) rot, ph, explored,
    the new memory, the reward, the loss and the minibatch indices."""
    import torch
    from antsrl_amd.population import PopulationMemoryAgent
    whole, shards = make_envs(s["P"], s["Em"], s["N"], s["max_time"], s["bf16"])
    pop = PopulationMemoryAgent(members_of(s), mem_size=s["mem"], power=s["power"], state_memory=state_memory,
                                record_per_step=s["K"], replay_size=s["ring"], minibatch=s["B"], min_replay=s["min_replay"],
                                update_target_every=1, seed=3)
    pop.setup(whole)
    pop.initialize(whole)
    whole.observe()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # the fused loop reads nothing back
    log = []
    try:
        for t in range(s["steps"]):
            before = pop.trainer.step_count
            loss = pop.rollout_step(whole)
            trained = pop.trainer.step_count != before
            log.append(SimpleNamespace(rot=pop._rot.clone(), ph=pop._ph.clone(), explored=pop._explored.clone(),
                                       mem=pop.previous_memory.clone(), reward=whole.reward.clone(), loss=loss,
                                       idx=pop.trainer.last_idx if trained else None))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return SimpleNamespace(pop=pop, env=whole, shards=shards, log=log)


def run_member_alone(s, p, run, state_memory):
    """Member p alone on its shard handle, entry by entry; every step's outputs are compared as it goes.  Returns the
    member's trainer, ring and two memory halves (the current one first)."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.replay import DeviceReplayMemory
    from antsrl_amd.train import MemoryTrainer
    lib = _lib.load()
    Em, N, mem = s["Em"], s["N"], s["mem"]
    Mm, env = Em * N, run.shards[p]
    seed, eps = s["seed"][p], s["epsilon"][p]
    tr = MemoryTrainer(F, env.device, discount=s["discount"][p], lr=s["lr"][p], update_target_every=1, power=s["power"],
                       mem_size=mem, seed=seed)
    rm = DeviceReplayMemory(s["ring"], (7, 7, 6), [2 + mem], [2], device=env.device)
    env.set_activation(torch.full((Em, N, env.cfg.n_phero), 10.0, device=env.device))
    env.observe()
    explored = torch.zeros((Em,), dtype=torch.uint8, device=env.device)
    halves, cur = [torch.zeros((Mm, mem), device=env.device) for _ in range(2)], 0
    rows, envs = slice(p * Mm, (p + 1) * Mm), slice(p * Em, (p + 1) * Em)
    for t, want in enumerate(run.log):
        obs, ast = env.obs, env.agent_state
        old, new = halves[cur], halves[1 - cur]
        rot, ph, _ = tr.policy.act(obs, ast, memory=old, out=new, env=env)
        rot, ph = rot.reshape(-1).clone(), ph.reshape(-1).clone()
        _lib.check(lib.antsrl_agent_select(seed, t, p * Em, Em, N, eps, 3, 3, mem, ptr(rot), ptr(ph), ptr(old), ptr(new),
                                           ptr(explored), stream()), "agent_select")
        cur = 1 - cur
        assert torch.equal(rot, want.rot[rows]), ("rot", p, t)
        assert torch.equal(ph, want.ph[rows]), ("ph", p, t)
        assert torch.equal(explored, want.explored[envs]), ("explored", p, t)
        assert torch.equal(new, want.mem[rows]), ("the new memory", p, t)
        rm.record_pre(obs, ast, new if state_memory == "reference" else old, rot, ph, n_envs=Em, n_ants=N, k=s["K"], seed=seed,
                      step=t, env_id_base=p * Em)
        done = env.query(cm.Q_TIMESTEP) == s["max_time"]
        env.step_update(rot.view(Em, N), ph.view(Em, N))
        rm.record_post(env.obs, env.agent_state, new, env.reward.view(-1), env.done)
        assert torch.equal(env.reward.view(-1), want.reward.view(-1)[rows]), ("reward", p, t)
        if rm.fill >= s["min_replay"]:
            assert want.idx is not None, ("the population did not train at step", t)
            loss = tr.train_on(rm, want.idx[p], done)
            assert torch.equal(loss, want.loss[p]), ("loss", p, t, float(loss), float(want.loss[p]))
        else:
            assert want.idx is None and not torch.is_tensor(want.loss) and want.loss == 0, ("the population trained at step", t)
    return tr, rm, (halves[cur], halves[1 - cur])


def same_member(pop, p, tr, rm, halves):
    """At the end: the ring's seven arrays with head and fill, both state blocks byte for byte (masters, Adam's moments,
    the training packs), the acting pack, the gradients, the dicts, the counters and both memory halves."""
    import torch
    t, Mm = pop.trainer, pop.g.Mm
    same_rings(pop.replay_memory.member(p), rm, RING)
    assert torch.equal(t._model[p], tr._model), ("the model's state block", p)
    assert torch.equal(t._target[p], tr._target), ("the target's state block", p)
    assert torch.equal(t.packed[p], tr.policy.packed), ("the acting pack", p)
    assert torch.equal(t.grads[p], tr.grads), ("grads", p)
    sd, alone = t.state_dict(p), tr.state_dict()
    assert list(sd) == list(alone) and len(sd) == 26 and all(torch.equal(sd[k], alone[k]) for k in sd)
    td, alone = t.target_state_dict(p), tr.target_state_dict()
    assert all(torch.equal(td[k], alone[k]) for k in td)
    ad, alone = t.adam_state(p), tr.adam_state()
    assert ad["step"] == alone["step"] and all(torch.equal(ad[m][k], alone[m][k]) for m in ("exp_avg", "exp_avg_sq") for k in ad[m])
    assert (t.step_count, t.syncs) == (tr.step_count, tr.syncs), ((t.step_count, t.syncs), (tr.step_count, tr.syncs))
    rows = slice(p * Mm, (p + 1) * Mm)
    assert torch.equal(pop._mem[pop._cur][rows], halves[0]) and torch.equal(pop._mem[1 - pop._cur][rows], halves[1])


def checked_run(name, state_memory="reference"):
    """The run of SHAPES[name] with every member checked against its lone run, once per session."""
    key = (name, state_memory)
    if key not in _RUNS:
        s = SHAPES[name]
        run = run_population(s, state_memory)
        for p in range(s["P"]):
            same_member(run.pop, p, *run_member_alone(s, p, run, state_memory))
        t, ring = run.pop.trainer, run.pop.replay_memory
        run.final = SimpleNamespace(step_count=t.step_count, syncs=t.syncs, fill=ring.fill, head=ring.head, model=t._model.clone(),
                                    agent_states=ring.agent_states.clone(), new_agent_states=ring.new_agent_states.clone())
        _RUNS[key] = run
    return _RUNS[key]


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
    run = checked_run("a")
    pop = run.pop
    tr, rm, Mm = pop.trainer, pop.replay_memory, pop.g.Mm
    rows = lambda p: slice(p * Mm, (p + 1) * Mm)  # noqa: E731
    weights = lambda p: [t[p].clone() for t in (tr._model, tr._target, tr.packed)]  # noqa: E731
    memory = lambda p: [m[rows(p)].clone() for m in pop._mem]  # noqa: E731
    slab = lambda p: [getattr(rm, n)[p].clone() for n in RING]  # noqa: E731
    same = lambda xs, ys: all(torch.equal(a, b) for a, b in zip(xs, ys))  # noqa: E731
    # the memory halves of the members differ: member 2 always explored (zero), member 0 never did
    pop._mem[pop._cur][rows(2)].uniform_(-1, 1)
    before_w, before_m, before_s = ([f(p) for p in range(3)] for f in (weights, memory, slab))
    assert not same(before_w[0], before_w[2]) and not same(before_m[0], before_m[2]) and not same(before_s[0], before_s[2])
    pop.copy_member(0, 2, ring=False)
    assert same(weights(2), before_w[0]) and same(memory(2), before_m[0]), "weights, Adam, target, pack and memory are member 0's"
    assert same(slab(2), before_s[2]), "with ring=False the slab stays"
    pop.copy_member(0, 2)
    assert same(weights(2), before_w[0]) and same(memory(2), before_m[0]) and same(slab(2), before_s[0])
    for p in (0, 1):
        assert same(weights(p), before_w[p]) and same(memory(p), before_m[p]) and same(slab(p), before_s[p]), "member %d changed" % p
    assert list(pop.epsilon) == [0.0, 0.5, 1.0]  # the hyper-parameters stay the member's own
    loss = pop.rollout_step(run.env)
    assert loss.shape == (3,) and bool(torch.isfinite(loss).all())


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
