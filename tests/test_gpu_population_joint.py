"""PopulationJointAgent, the curriculum's third stage for a sweep (antsrl_amd/population.py; include/antsrl.h, "The
population of joint agents"; antsrl_popjoint.hip) on the device.

1. The population equals its members: member p is, bit for bit, CollectAgent(train_layer1=True)'s entries (JointTrainer
   and its acting policy) run alone on a shard handle of its Em environments with the member's own seed, epsilon,
   discount and learning rate — actions, explored flags, rewards and loss after every step; the ring, the model blocks,
   the target layer3, both Adam moments, gradients, the dicts and the counters at the end (population_harness.py holds
   the two shapes and the comparison).
2. Acting: antsrl_pop_joint_policy on flat blocks against antsrl_pop_policy on the same weights as separate tensors.
3. The hand-over from a PopulationAgent: load_collect_population against the per-member state_dict route.
4. copy_member.
5. driver.train_population_curriculum with three stages, and the two-stage call as it was.
(The training step alone: test_gpu_population_joint_stages.py.)"""
import ctypes as C

import numpy as np
import pytest

import population_stage_cases as S
from agent_harness import ptr, stream
from population_harness import _A, _B, RING, Kind, population_trainer, synthetic_ring

pytestmark = pytest.mark.gpu

#: (a) is the harness's _A: B = 48, one forward workgroup, bfloat16.  (b) is _B with B = 136: two forward workgroups, the
#: second with one tile of 8 valid rows, float32
SHAPES = dict(a=_A, b=dict(_B, B=136))
JOINT = Kind("PopulationJointAgent", "JointTrainer", True, "model", SHAPES,
             lambda t, p, tr: (("model", t.model[p], tr.model), ("target_l3", t.target_l3[p], tr.target_l3),
                               ("adam m", t._adam[0, p], tr._adam[0]), ("adam v", t._adam[1, p], tr._adam[1]),
                               ("grads", t.grads[p], tr.grads)))
H = JOINT

PATTERN, GUARD = 0xA5, 256


def test_the_kind_is_the_issue_s():
    assert (H.population, H.single, H.pheromone, H.final) == ("PopulationJointAgent", "JointTrainer", True, "model")
    assert SHAPES["a"] is _A and SHAPES["a"]["B"] == 48 and SHAPES["a"]["bf16"]
    assert SHAPES["b"] == dict(_B, B=136) and not SHAPES["b"]["bf16"] and ((136 + 31) // 32 + 3) // 4 == 2 and 136 - 4 * 32 == 8


# ---- 1. the population equals its members
@pytest.mark.parametrize("name", ["a", "b"])
def test_the_population_equals_its_members(name):
    import torch
    s = H.SHAPES[name]
    run = H.checked_run(name)  # every comparison of the module docstring's point 1 is made in there
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
    ph = torch.stack([w.ph for w in run.log]).view(s["steps"], P, -1)
    for p in range(P):
        for q in range(p + 1, P):
            assert not torch.equal(rot[:, p], rot[:, q]) and not torch.equal(ph[:, p], ph[:, q]), (p, q)
            assert not torch.equal(end.model[p], end.model[q]), (p, q)
    losses = torch.stack([w.loss for w in run.log if torch.is_tensor(w.loss)])
    assert losses.shape == (end.step_count, P) and bool(torch.isfinite(losses).all())
    # layer1 is trained: every member's w1 has left its initialisation
    fresh = population_trainer("PopulationJointTrainer", P, (7, 7, 6), run.env.device, s["seed"], s["discount"], s["lr"])
    n1 = 32 * 296
    for p in range(P):
        assert not torch.equal(end.model[p, :n1], fresh.model[p, :n1]), ("w1 did not move", p)


# ---- 2. acting
@pytest.mark.parametrize("name", S.ACTING_IDS)
def test_acting(name):
    """antsrl_pop_joint_policy on the members' flat blocks (w1 | b1 | w2 | b2 | the LIVE w3 | b3) and target layer3
    against antsrl_pop_policy on the same weights as separate tensors: rotation and pheromone bit for bit, in both
    observation formats.  acting_inputs' target layer3 differs from the live one in the block, so reading layer3 from the
    block would show.  No tolerance is involved."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.population import _Geometry
    lib = _lib.load()
    c = S.acting_case(name)
    inp, P, Em, N, Mm, F = c["inp"], c["P"], c["Em"], c["N"], c["Mm"], c["F"]
    dev = lambda t: t.cuda().contiguous()  # noqa: E731
    w1, b1, ast = dev(inp["w1"]), dev(inp["b1"]), dev(inp["ast"].reshape(P * Mm, 2))
    heads = dev(torch.cat([inp["w2"].reshape(P, -1), inp["b2"], inp["w3"].reshape(P, -1), inp["b3"]], 1))
    target_l3 = dev(torch.cat([inp["tw3"].reshape(P, -1), inp["tb3"]], 1))
    blocks = dev(torch.cat([inp["w1"].reshape(P, -1), inp["b1"], heads.cpu()], 1))
    assert blocks.shape == (P, 32 * (F + 2) + 230) and target_l3.shape == (P, 99)
    assert not bool((target_l3 == blocks[:, -99:]).all(dim=1).any()), "a target layer3 that differs from the live one"

    def guarded():
        buf = torch.full((GUARD + P * Mm + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        return buf, buf[GUARD:GUARD + P * Mm].view(torch.int8)

    zeros = [0] * P
    got = {}
    for dtype in (torch.float32, torch.bfloat16):
        obs = dev(inp["obs"].reshape(P * Mm, F)).to(dtype)
        assert obs.data_ptr() % 16 == 0
        spec = _Geometry(P, P * Em, N, 0, F, dtype).spec(zeros, zeros, [1e-4] * P, zeros)
        (rbuf, rot), (pbuf, ph) = guarded(), guarded()
        _lib.check(lib.antsrl_pop_joint_policy(C.byref(spec), ptr(obs), ptr(ast), ptr(blocks), ptr(target_l3), ptr(rot), ptr(ph),
                                               stream()), "pop_joint_policy")
        (_, rot0), (_, ph0) = guarded(), guarded()
        _lib.check(lib.antsrl_pop_policy(C.byref(spec), ptr(obs), ptr(ast), ptr(w1), ptr(b1), ptr(heads), ptr(target_l3), ptr(rot0),
                                         ptr(ph0), stream()), "pop_policy")
        torch.cuda.synchronize()
        for buf, what in ((rbuf, "rot"), (pbuf, "ph")):
            assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + P * Mm:] == PATTERN).all()), ("the guards of " + what, dtype)
        assert torch.equal(rot, rot0), ("rot", dtype, int((rot != rot0).sum()))
        assert torch.equal(ph, ph0), ("ph", dtype, int((ph != ph0).sum()))
        assert int(rot.min()) >= -1 and int(rot.max()) <= 1 and int(ph.min()) >= 0 and int(ph.max()) <= 2
        # the float64 net's first maximum on every clear row (the cases' own reference, with the TARGET layer3)
        for p in range(P):
            rows, clear = slice(p * Mm, (p + 1) * Mm), c["clear"][p]
            assert torch.equal(rot[rows].cpu().long()[clear[:, 0]], c["rot"][p][clear[:, 0]]), ("rot against float64", p, dtype)
            assert torch.equal(ph[rows].cpu().long()[clear[:, 1]], c["ph"][p][clear[:, 1]]), ("ph against float64", p, dtype)
        got[dtype] = (rot.clone(), ph.clone())
    a, b = got[torch.float32], got[torch.bfloat16]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "both observation formats give equal actions"


# ---- 3. the hand-over
def test_hand_over():
    import torch
    from antsrl_amd.population import PopulationAgent, PopulationJointAgent
    from antsrl_amd.train import JointTrainer
    s = SHAPES["b"]
    P, F, B = s["P"], 294, 40
    env, _ = H.make_envs(P, s["Em"], s["N"], 50, False)
    members = H.members_of(s)
    pop_c = PopulationAgent(members, replay_size=100, minibatch=32, min_replay=64, seed=3)
    pop_c.setup(env)
    ring = synthetic_ring(P, 256, (7, 7, 6), env.device, seed=4)
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    for _ in range(3):  # stage 2 has trained and not synced since: its target layer3 is not its live one
        pop_c.trainer.step(ring, torch.randint(0, 256, (P, 32), generator=g).to(env.device))
    ct = pop_c.trainer
    assert not torch.equal(ct.target_l3, ct.heads[:, 99:])
    before = [t.clone() for t in (ct.w1, ct.b1, ct.heads, ct.target_l3, ct._adam)]
    new = lambda: PopulationJointAgent(members, replay_size=100, minibatch=B, min_replay=64, seed=3)  # noqa: E731
    plain, by_dict, pop_j = new(), new(), new()
    plain.setup(env)
    by_dict.setup(env)
    for p in range(P):
        by_dict.trainer.load_state_dict(ct.state_dict(p), p)
    pop_j.setup(env, collect_population=pop_c)
    assert all(torch.equal(a, b) for a, b in zip(before, (ct.w1, ct.b1, ct.heads, ct.target_l3, ct._adam))), \
        "the hand-over reads the collect population"
    t, d, fresh, n1 = pop_j.trainer, by_dict.trainer, plain.trainer, 32 * (F + 2)
    assert torch.equal(t.model, d.model) and torch.equal(t.target_l3, d.target_l3) and torch.equal(t._adam, d._adam)
    for p in range(P):
        assert torch.equal(t.model[p, :n1], ct.w1[p].reshape(-1)) and torch.equal(t.model[p, n1:n1 + 32], ct.b1[p]), p
        assert torch.equal(t.model[p, n1 + 32:], ct.heads[p]) and torch.equal(t.target_l3[p], ct.heads[p, 99:]), p
        assert not torch.equal(t.model[p, n1 + 32:], fresh.model[p, n1 + 32:]), "the collect population has trained"
    assert not bool(t._adam.any()) and t.step_count == 0, "Adam stays zero"
    # one step afterwards is the lone JointTrainer's, loaded from the same dict
    idx = torch.randint(0, 256, (P, B), generator=g).to(env.device)
    loss = t.step(ring, idx)
    for p in range(P):
        one = JointTrainer(F, env.device, discount=members[p]["discount"], lr=members[p]["learning_rate"], update_target_every=1000,
                           seed=members[p]["seed"], state_dict=ct.state_dict(p))
        l1 = one.step(tuple(getattr(ring, n)[p] for n in RING), idx[p])
        assert torch.equal(l1, loss[p]), ("loss", p, float(l1), float(loss[p]))
        H.same_trainers(t, p, one)
    # unequal member counts and widths, in load_explore_population's words
    with pytest.raises(ValueError, match="the collect population has 2 members, this one 1"):
        PopulationJointAgent(members[:1]).setup(env, collect_population=pop_c)
    narrow = population_trainer("PopulationLinearTrainer", P, (5, 5, 2), env.device, s["seed"], s["discount"], s["lr"])
    with pytest.raises(ValueError, match="the collect population's rows have 50 features, these 294"):
        t.load_collect_population(narrow)


# ---- 4. copy_member
def test_copy_member():
    import torch
    tr = H.checked_run("a").pop.trainer
    weights = lambda p: [t.clone() for t in (tr.model[p], tr.target_l3[p], tr._adam[:, p])]  # noqa: E731
    before_w = [weights(p) for p in range(3)]
    assert not torch.equal(before_w[0][0], before_w[2][0])
    H.check_copy_member(weights, "model, target layer3 and Adam are member 0's")  # the other assertions are the harness's


# ---- 5. the curriculum
def test_train_population_curriculum():
    """P = 2, Em = 1, 32 ants, 1 + 1 + 1 episodes of 6 steps; 32 rows per step against min_replay = 64: each stage trains
    from its second step on.  Then the two-stage call, as it was."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.driver import episode_seed, train_population_curriculum
    from antsrl_amd.population import PopulationAgent, PopulationExploreAgent, PopulationJointAgent
    P, N, EPISODES, STEPS, SEED = 2, 32, (1, 1, 1), 6, 21
    env, _ = H.make_envs(P, 1, N, STEPS, False)
    members = [dict(epsilon=0.5, discount=0.5, learning_rate=1e-3, seed=7), dict(epsilon=0.9, discount=0.99, learning_rate=1e-4, seed=9)]
    kw = dict(replay_size=300, minibatch=32, min_replay=64)
    pop_e, pop_c, pop_j = PopulationExploreAgent(members, seed=3, **kw), PopulationAgent(members, seed=4, **kw), PopulationJointAgent(members, seed=5, **kw)
    gen = cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)
    seeds, generate = [], env.generate

    def watched_generate(g, seed):
        seeds.append(seed)
        return generate(g, seed)
    env.generate = watched_generate
    handed, fused = {}, pop_j.rollout_step

    def first_step(e, training=True):
        if not handed:  # stage 3's first step: what the hand-over left, and stage 2's final tensors
            handed.update(model=pop_j.trainer.model.clone(), target_l3=pop_j.trainer.target_l3.clone(),
                          steps_c=pop_c.trainer.step_count, steps_j=pop_j.trainer.step_count)
        return fused(e, training)
    pop_j.rollout_step = first_step
    logs = train_population_curriculum(pop_e, pop_c, env, gen, EPISODES, STEPS, seed=SEED, report_every=STEPS, joint_pop=pop_j)
    assert isinstance(logs, tuple) and len(logs) == 3
    log1, log2, log3 = logs
    for pop in (pop_e, pop_c, pop_j):
        assert pop.trainer.step_count == STEPS - 1, (pop.name, pop.trainer.step_count)
    for log in logs:
        assert log["member_loss"].shape == (1, P) and np.isfinite(log["member_loss"]).all(), log["member_loss"]
        assert log["member_total"].shape == (1, P) and log["monitor"] is log1["monitor"]
    assert list(log3["report_episode"]) == [0, 1, 2]  # one monitor: three episodes' reports
    # the seeds continue: stage k's episodes start from seed + the episodes before it (the first map is generated twice:
    # once for stage 1's setup, once by its first episode)
    want_seeds = [episode_seed(env.cfg, gen, SEED + k, 0) for k in range(3)]
    assert seeds == want_seeds[:1] + want_seeds and len(set(seeds)) == 3
    # the hand-overs: stage 2 froze stage 1's final layer1; stage 3 started from stage 2's final six tensors
    n1, ct, et = 32 * 296, pop_c.trainer, pop_e.trainer
    assert torch.equal(ct.w1.view(P, n1), et.model[:, :n1])
    assert handed["steps_c"] == ct.step_count and handed["steps_j"] == 0
    want = torch.cat([ct.w1.view(P, n1), ct.b1, ct.heads], 1)
    assert torch.equal(handed["model"], want) and torch.equal(handed["target_l3"], ct.heads[:, 99:])
    assert not torch.equal(pop_j.trainer.model[:, :n1], handed["model"][:, :n1]), "stage 3 trains layer1"

    # without joint_pop nothing changed: two entries, two logs
    pop_e2, pop_c2 = PopulationExploreAgent(members, seed=3, **kw), PopulationAgent(members, seed=4, **kw)
    del seeds[:]
    two = train_population_curriculum(pop_e2, pop_c2, env, gen, EPISODES[:2], STEPS, seed=SEED, report_every=STEPS)
    assert isinstance(two, tuple) and len(two) == 2 and seeds == want_seeds[:1] + want_seeds[:2]
    assert np.array_equal(two[0]["member_loss"], log1["member_loss"]) and np.array_equal(two[1]["member_loss"], log2["member_loss"])
