"""PopulationExploreAgent and its hand-over to PopulationAgent (antsrl_amd/population.py; include/antsrl.h, "The population
of explore agents") on the device.

1. The population equals its members: member p is, bit for bit, an ExploreAgent's entries run alone on a shard handle of
   its Em environments with the member's own seed, epsilon, discount and learning rate — actions, explored flags,
   rewards and loss after every step; the ring, the model and target blocks, Adam's moments, gradients and counters at the
   end (population_harness.py holds the two shapes and the comparison).
2. The step alone: PopulationExploreTrainer.step against P ExploreTrainer.steps on the same synthetic rows, over the
   widths and minibatches at which the kernels take another path; the running loss; equal bits for equal inputs; the
   members' parts of the workspace.
3. Acting uses the target block.
4. The hand-over: layer1 and layer2 of every member into a PopulationAgent, device to device.
5. copy_member.
6. driver.train_population_curriculum: both stages on one handle and monitor, no host read inside an episode."""
from functools import partial

import numpy as np
import pytest

from population_harness import EXPLORE as H
from population_harness import RING, synthetic_ring
from population_harness import population_trainer as _population_trainer

population_trainer = partial(_population_trainer, "PopulationExploreTrainer")  # (P, space, device, seeds, discount, lr)

pytestmark = pytest.mark.gpu


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
    # members that share a seed differ through their environment ids (and members at large differ at all)
    rot = torch.stack([w.rot for w in run.log]).view(s["steps"], P, -1)
    for p in range(P):
        for q in range(p + 1, P):
            assert not torch.equal(rot[:, p], rot[:, q]), (p, q)
            assert not torch.equal(end.model[p], end.model[q]), (p, q)
    losses = torch.stack([w.loss for w in run.log if torch.is_tensor(w.loss)])
    assert losses.shape == (end.step_count, P) and bool(torch.isfinite(losses).all())


# ---- 2. the step alone
@pytest.mark.parametrize("space", [(7, 7, 6), (5, 5, 2)], ids=["F294", "F50"])
@pytest.mark.parametrize("B", [1, 33, 136, 512])
def test_the_step_alone(space, B):
    """F = 294 is the agents'; F = 50 has F + 3 = 53 columns, so the last layer1 slab has columns beyond the product,
    F % 16 != 0 (a partial k-step) and a member's block of 32 * 52 + 131 = 1795 floats is odd.  B = 1: one row; 33: a
    whole tile and one row of the next; 136: two forward workgroups per member; 512: the limit, four."""
    import ctypes as C
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.train import ExploreTrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    P, L, F = 3, 600, int(np.prod(space))
    seeds, discount, lr = (7, 8, 7), (0.5, 0.99, 0.9), (1e-3, 1e-4, 3e-3)
    ring = synthetic_ring(P, L, space, dev, seed=11)
    g = torch.Generator(device="cpu")
    g.manual_seed(B)
    idx = [torch.randint(0, L, (P, B), generator=g).to(dev) for _ in range(2)]

    def run():
        """Two consecutive steps; the workspace is one filled with a pattern, with a guard behind it."""
        tr = population_trainer(P, space, dev, seeds, discount, lr)
        tf, stride, ws, launches = tr._sizes(B)
        assert tf == 32 * (F + 2) + 131 and tf % 2 == 1 and launches == 2 and ws == P * stride and stride % 256 == 0
        big = torch.full((ws + 1024,), 0xA5, dtype=torch.uint8, device=dev)
        tr._work, tr._work_B = big[:ws], B
        assert big.data_ptr() % 256 == 0
        losses = [tr.step(ring, idx[0]).clone()]
        first = dict(model=tr.model.clone(), grads=tr.grads.clone(), adam=tr._adam.clone(), rl=tr.running_loss.clone())
        losses.append(tr.step(ring, idx[1]).clone())
        return tr, big, stride, losses, first

    tr, big, stride, losses, first = run()
    assert torch.equal(first["rl"], losses[0].double()), "the first training step's running loss is its loss"
    # main.py:106-109 in float64, each product rounded before the add (antsrl_monitor.hip's arithmetic)
    assert torch.equal(tr.running_loss, 0.99 * losses[0].double() + 0.01 * losses[1].double())
    assert bool(torch.isfinite(torch.stack(losses)).all()) and not torch.equal(first["model"], tr.model)
    assert torch.equal(tr.target, population_trainer(P, space, dev, seeds, discount, lr).target), "a step leaves the target"

    # every member against an ExploreTrainer of its own on its slab
    single_bytes = C.c_size_t()
    _lib.check(_lib.load().antsrl_exptrain_sizes(F, B, None, C.byref(single_bytes), None), "exptrain_sizes")
    blocks = ((B + 31) // 32 + 3) // 4
    dh_off = (blocks * 104 * 4 + 255) // 256 * 256
    assert single_bytes.value == dh_off + B * 128 <= stride
    for p in range(P):
        one = ExploreTrainer(F, dev, discount=discount[p], lr=lr[p], update_target_every=1000, seed=seeds[p])
        slab = tuple(getattr(ring, n)[p] for n in RING)
        l0 = one.step(slab, idx[0][p])
        assert torch.equal(l0, losses[0][p]), ("loss", p, 0, float(l0), float(losses[0][p]))
        for name, mine, alone in (("model", first["model"][p], one.model), ("grads", first["grads"][p], one.grads),
                                  ("adam m", first["adam"][0, p], one._adam[0]), ("adam v", first["adam"][1, p], one._adam[1])):
            assert torch.equal(mine, alone), (name, p, "after the first step")
        l1 = one.step(slab, idx[1][p])  # on the weights and moments the first step moved
        assert torch.equal(l1, losses[1][p]), ("loss", p, 1, float(l1), float(losses[1][p]))
        H.same_trainers(tr, p, one)
        assert tr.step_count == one.step_count == 2
        # the member's part of the workspace: dh is the single step's, and what neither stage writes kept the pattern —
        # the gap between the partials and dh, and the stride's tail behind dh
        part = big[p * stride:(p + 1) * stride]
        assert torch.equal(part[dh_off:dh_off + B * 128], one._work[dh_off:dh_off + B * 128]), ("dh", p)
        assert bool((part[blocks * 104 * 4:dh_off] == 0xA5).all()), ("the gap in front of dh", p)
        assert bool((part[single_bytes.value:] == 0xA5).all()), ("the stride's tail", p)
    assert bool((big[P * stride:] == 0xA5).all()), "the guard behind the workspace"

    # equal inputs give equal bits
    tr2, _, _, losses2, first2 = run()
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    for a, b in ((tr.model, tr2.model), (tr.grads, tr2.grads), (tr._adam, tr2._adam), (tr.running_loss, tr2.running_loss),
                 (first["model"], first2["model"])):
        assert torch.equal(a, b)


# ---- 3. acting uses the target block
def test_acting_uses_the_target_block():
    import torch
    from antsrl_amd.policy import LinearPolicy
    from antsrl_amd.population import PopulationExploreAgent
    P, Em, N = 2, 1, 32
    env, _ = H.make_envs(P, Em, N, 50, False)
    pop = PopulationExploreAgent([dict(epsilon=0.5, discount=0.5, learning_rate=5e-2, seed=7),
                                  dict(epsilon=0.5, discount=0.9, learning_rate=5e-2, seed=9)], replay_size=256, minibatch=64)
    pop.setup(env)
    pop.initialize(env)
    env.observe()
    act = lambda: pop.get_action(env.obs, env.agent_state, training=False)  # noqa: E731
    rot, none = act()
    assert none is None and rot.shape == (P * Em, N) and rot.dtype == torch.int8
    before = rot.clone()
    ring = synthetic_ring(P, 256, (7, 7, 6), env.device, seed=4)
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    target = pop.trainer.target.clone()
    for _ in range(3):  # three steps at a learning rate of 0.05 move every weight by many bfloat16 ulps
        pop.trainer.step(ring, torch.randint(0, 256, (P, 64), generator=g).to(env.device))
    assert torch.equal(pop.trainer.target, target) and not torch.equal(pop.trainer.model, target)
    assert torch.equal(act()[0], before), "a training step without a sync leaves the actions"
    pop.trainer.sync_target()
    assert torch.equal(pop.trainer.target, pop.trainer.model) and pop.trainer.syncs == 1
    after = act()[0].clone()
    for p in range(P):  # the single policy on the member's new target
        one = LinearPolicy(294, env.device, with_pheromone_head=False)
        one.load_state_dict(pop.trainer.target_state_dict(p))
        rows = slice(p * Em, (p + 1) * Em)
        want, ph = one.act(env.obs[rows].contiguous(), env.agent_state[rows].contiguous())
        assert ph is None and torch.equal(after[rows], want.view(Em, N)), p


# ---- 4. the hand-over
def test_hand_over(tmp_path):
    import torch
    from antsrl_amd.agent import CollectAgent
    from antsrl_amd.population import PopulationAgent
    s = H.SHAPES["b"]
    run = H.checked_run("b")
    pop_e, P, F = run.pop, s["P"], 294
    assert pop_e.trainer.step_count > 0
    members = H.members_of(s)
    new = lambda: PopulationAgent(members, replay_size=100, minibatch=32, min_replay=64, seed=3)  # noqa: E731
    plain, pop_c = new(), new()
    plain.setup(run.env)
    model_before = pop_e.trainer.model.clone()
    pop_c.setup(run.env, explore_population=pop_e)
    assert torch.equal(pop_e.trainer.model, model_before), "the hand-over reads the explore population"
    t, fresh, n1 = pop_c.trainer, plain.trainer, 32 * (F + 2)
    for p in range(P):
        block = pop_e.trainer.model[p]
        assert torch.equal(t.w1[p].reshape(-1), block[:n1]) and torch.equal(t.b1[p], block[n1:n1 + 32]), p
        assert torch.equal(t.heads[p, :99], block[n1 + 32:]), p
        assert not torch.equal(t.w1[p], fresh.w1[p]), "the explore population has trained"
    assert torch.equal(t.heads[:, 99:], fresh.heads[:, 99:]) and torch.equal(t.target_l3, fresh.target_l3), "layer3 and its target copy stay"
    assert torch.equal(t._adam, fresh._adam) and t.step_count == 0, "Adam's state stays"
    # the whole member is a CollectAgent set up from the member's saved file, with the member's seed
    for p in range(P):
        f = str(tmp_path / ("explore_%d.pt" % p))
        pop_e.save_model(p, f)
        assert list(torch.load(f)) == ["layer1.weight", "layer1.bias", "layer2.weight", "layer2.bias"]
        one = CollectAgent(members[p]["epsilon"], members[p]["discount"], learning_rate=members[p]["learning_rate"],
                           seed=members[p]["seed"], replay_size=100)
        one.setup(run.shards[p], explore_model=f)
        ot = one.trainer
        for name, mine, alone in (("w1", t.w1[p], ot.policy.w1), ("b1", t.b1[p], ot.policy.b1), ("heads", t.heads[p], ot.heads),
                                  ("target_l3", t.target_l3[p], ot.target_l3), ("adam", t._adam[p], ot._adam)):
            assert torch.equal(mine, alone), (name, p)
    # unequal member counts
    with pytest.raises(ValueError, match="2 members, this one 1"):
        PopulationAgent(members[:1]).setup(run.env, explore_population=pop_e)


# ---- 5. copy_member
def test_copy_member():
    import torch
    tr = H.checked_run("a").pop.trainer
    weights = lambda p: [t.clone() for t in (tr.model[p], tr.target[p], tr._adam[:, p])]  # noqa: E731
    before_w = [weights(p) for p in range(3)]
    assert not torch.equal(before_w[0][0], before_w[2][0])
    H.check_copy_member(weights, "model, target and Adam are member 0's")  # the other assertions are the harness's


# ---- 6. the curriculum
def test_train_population_curriculum(monkeypatch):
    """P = 2, Em = 1, 32 ants, 2 + 2 episodes of 10 steps; 32 rows per step against min_replay = 96: each stage trains
    from its third step on."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.driver import epsilon_schedule, train_population_curriculum
    from antsrl_amd.monitor import EpisodeMonitor
    from antsrl_amd.population import PopulationAgent, PopulationExploreAgent
    P, N, EPISODES, STEPS = 2, 32, (2, 2), 10
    env, _ = H.make_envs(P, 1, N, STEPS, False)
    members = [dict(epsilon=0.5, discount=0.5, learning_rate=1e-3, seed=7), dict(epsilon=0.9, discount=0.99, learning_rate=1e-4, seed=9)]
    pop_e = PopulationExploreAgent(members, replay_size=300, minibatch=32, min_replay=96, seed=3)
    pop_c = PopulationAgent(members, replay_size=300, minibatch=32, min_replay=96, seed=4)
    end = EpisodeMonitor.end_episode
    seen = {id(pop_e): [], id(pop_c): []}
    handed = {}

    def watch(pop):
        fused = pop.rollout_step

        def step(e, training=True):
            if pop is pop_c and not handed:  # stage 2's first step: what the hand-over left, and stage 1's final model
                handed.update(w1=pop_c.trainer.w1.clone(), model=pop_e.trainer.model.clone(), steps_e=pop_e.trainer.step_count)
            torch.cuda.set_sync_debug_mode("error")  # from here to the episode's end every host read is an error
            loss = fused(e, training)
            seen[id(pop)].append(loss)
            return loss
        pop.rollout_step = step

    def end_episode(self):
        end(self)
        torch.cuda.set_sync_debug_mode(0)
    watch(pop_e)
    watch(pop_c)
    monkeypatch.setattr(EpisodeMonitor, "end_episode", end_episode)
    gen = cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)
    lo, hi = np.array([0.01, 0.3]), np.array([1.0, 0.6])
    try:
        log1, log2 = train_population_curriculum(pop_e, pop_c, env, gen, EPISODES, STEPS, seed=21, min_epsilon=lo,
                                                 max_epsilon=hi, report_every=STEPS)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    monkeypatch.undo()
    for pop, episodes in ((pop_e, EPISODES[0]), (pop_c, EPISODES[1])):
        losses = seen[id(pop)]
        assert len(losses) == episodes * STEPS
        assert [torch.is_tensor(l) for l in losses[:STEPS]] == [False, False] + [True] * (STEPS - 2), "training starts at step 3"
        assert pop.trainer.step_count == episodes * STEPS - 2
    # member_loss is finite from the first training episode on (which is the stage's first), and the members' differ
    for log in (log1, log2):
        assert log["member_loss"].shape == (2, P) and np.isfinite(log["member_loss"]).all(), log["member_loss"]
        assert not np.array_equal(log["member_loss"][:, 0], log["member_loss"][:, 1])
        assert log["member_total"].shape == (2, P) and log["monitor"] is log1["monitor"]
    # the last running loss is the recurrence over the stage's losses, in float64
    for pop, log in ((pop_e, log1), (pop_c, log2)):
        rl = None
        for l in (x for x in seen[id(pop)] if torch.is_tensor(x)):
            rl = l.double() if rl is None else 0.99 * rl + 0.01 * l.double()
        assert np.array_equal(log["member_loss"][-1], rl.cpu().numpy())
    # the epsilons: what each episode ran with, member by member; each stage starts from its members' own and follows
    # the schedule with the member's bounds
    want_eps = [[0.5, 0.9], [epsilon_schedule(0, lo[0], hi[0]), epsilon_schedule(0, lo[1], hi[1])]]
    assert np.array_equal(log1["epsilons"], np.array(want_eps)) and np.array_equal(log2["epsilons"], np.array(want_eps))
    for pop in (pop_e, pop_c):
        assert list(pop.epsilon) == [epsilon_schedule(1, lo[p], hi[p]) for p in range(P)]
    # the hand-over: stage 2 ran its first episode on stage 1's final layer1 (which it freezes)
    n1 = 32 * 296
    assert handed["steps_e"] == pop_e.trainer.step_count and torch.equal(handed["model"], pop_e.trainer.model)
    assert torch.equal(handed["w1"].view(P, n1), pop_e.trainer.model[:, :n1])
    assert torch.equal(pop_c.trainer.w1, handed["w1"]), "layer1 stays frozen in stage 2"
    # one monitor: four episodes' reports, the rewards of both stages
    assert len(log2["report_episode"]) == 4 and list(log2["report_episode"]) == [0, 1, 2, 3]
    assert np.array_equal(log2["member_total"].sum(axis=1), log2["reports"][2:, :, 0].sum(axis=1))
    assert np.array_equal(log1["member_total"].sum(axis=1), log2["reports"][:2, :, 0].sum(axis=1))
