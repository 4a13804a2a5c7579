"""What the device tests of the four populations share (test_gpu_population.py, _explore.py, _joint.py,
_memory_agent.py): the environment a population acts in with the shard handles of its members, a description of each
kind (COLLECT: PopulationAgent against LinearTrainer; EXPLORE: PopulationExploreAgent against ExploreTrainer and its
LinearPolicy without a pheromone head; MEMORY: PopulationMemoryAgent against MemoryTrainer with the carried memory; the
joint kind is built in its test file) with the two shapes of its acceptance test, and the comparison itself — a
population's fused loop against every member run ALONE on a shard handle of its own environments, driven entry by entry
as agent_harness.drive_loop drives an agent: one loop of each, whatever the net carries; and what the tests of a training
step alone share (a synthetic ring, a trainer without an agent).  torch is imported inside the functions, as in the GPU
test files."""
from types import SimpleNamespace

import numpy as np

from agent_harness import ptr, same_rings, stream

F = 294  # 7 x 7 x 6 observations
RING = ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")

#: the acceptance tests' two shapes.  (a): 40 ants per member, so its second tile has 8 rows, bfloat16 on the cell-meta
#: path; members 0 and 2 share a seed and must still differ through their environment ids; B = 48 is one whole tile and
#: half of one (ONE forward workgroup of the explore step); 40 rows per step wrap the 200-row ring in step 5.  (b):
#: float32; K = 24 is the stratified sample, and 24 rows per step wrap the 300-row ring at step 13.  Its B is the kind's:
#: 264 is the reference's nine tiles; 136 is five tiles, so an explore member has TWO forward workgroups, the second with
#: one tile of 8 valid rows, and the layer1 stage adds their partials in workgroup order.  max_time 8 gives an episode end
#: and a target sync inside either run.  slice_bytes (collect): a member's observation slice, asserted in run_population.
_A = dict(P=3, Em=2, N=20, bf16=True, epsilon=(0.0, 0.5, 1.0), lr=(1e-3, 1e-4, 3e-3), discount=(0.5, 0.99, 0.9),
          seed=(7, 8, 7), K=None, ring=200, min_replay=80, B=48, max_time=8, steps=14)
_B = dict(P=2, Em=1, N=32, bf16=False, epsilon=(0.5, 0.5), lr=(1e-3, 1e-3), discount=(0.5, 0.99), seed=(7, 9), K=24,
          ring=300, min_replay=48, max_time=8, steps=18)


def members_of(s):
    return [dict(epsilon=s["epsilon"][p], discount=s["discount"][p], learning_rate=s["lr"][p], seed=s["seed"][p])
            for p in range(s["P"])]


def make_envs(P, Em, N, max_time, bf16, init_seed=5):
    """The population's environment (P * Em colonies of N ants on 64 x 64 cells, 7 x 7 x 6 observations, synth_init as
    agent_harness.make_env does; bf16: bfloat16 observations on the cell-meta path) and, per member, a shard handle of its
    Em environments with env_id_base = p * Em, n_envs_total = E and the init's rows p * Em : (p + 1) * Em."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    E = P * Em
    kw = dict(deposit_strength=256.0, max_time=max_time)
    if bf16:
        kw["act_path"] = cm.ACT_CELL_META
    dtype = torch.bfloat16 if bf16 else torch.float32
    cfg = cm.make_cfg(E, N, 64, 64, **kw)
    init = synth_init(cfg, seed=init_seed, n_food_discs=6, food_rmin=3, food_rmax=6)
    whole = BatchedAntsEnv(cfg, obs_dtype=dtype)
    whole.reset(init)
    shards = []
    for p in range(P):
        env = BatchedAntsEnv(cm.make_cfg(Em, N, 64, 64, env_id_base=p * Em, n_envs_total=E, **kw), obs_dtype=dtype)
        env.reset({k: np.ascontiguousarray(v[p * Em:(p + 1) * Em]) for k, v in init.items()})
        shards.append(env)
    return whole, shards


# ---- a training step alone: test_gpu_population_explore.py's and test_gpu_population_stages.py's
def synthetic_ring(P, L, space, device, seed):
    """A PopulationReplayMemory of L full rows per member: random observations, agent states, actions in {0, 1, 2},
    rewards and a fifth of the rows done."""
    import torch
    from antsrl_amd.population import PopulationReplayMemory
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    ring = PopulationReplayMemory(P, L, space, device=device)
    r = lambda *shape: torch.rand(shape, generator=g)  # noqa: E731
    ring.states.copy_(r(P, L, *space) * 2 - 1)
    ring.new_states.copy_(r(P, L, *space) * 2 - 1)
    ring.agent_states.copy_(r(P, L, 2))
    ring.new_agent_states.copy_(r(P, L, 2))
    ring.actions.copy_(torch.randint(0, 3, (P, L, 2), generator=g))
    ring.rewards.copy_(r(P, L) * 4 - 2)
    ring.dones.copy_(r(P, L) < 0.2)
    ring.fill = L
    return ring


def population_trainer(cls, P, space, device, seeds, discount, lr):
    """A population trainer without an agent.  cls: "PopulationLinearTrainer" or "PopulationExploreTrainer"."""
    import torch
    from antsrl_amd import population
    F = int(np.prod(space))
    g = population._Geometry(P, P, 8, 0, F, torch.float32)  # the training entry reads the spec's members and n_features only
    return getattr(population, cls)(g, device, seeds, discount, lr, update_target_every=1000)


class Kind:
    """One kind of population.  population / single: the names of its agent class (antsrl_amd.population) and of the
    single agent's trainer (antsrl_amd.train); pheromone: whether the net has that head; final: the trainer tensor a
    run's `final` keeps a copy of; tensors(t, p, tr) -> the (name, member p's tensor of the population trainer t, the lone
    trainer tr's) that same_trainers compares.  A kind whose net carries more than the agent state (MemoryKind) overrides
    the hooks below the constructor; `variant` is what checked_run runs when it is given none."""

    make_envs, members_of = staticmethod(make_envs), staticmethod(members_of)
    variant = None

    def __init__(self, population, single, pheromone, final, SHAPES, tensors):
        self.population, self.single, self.pheromone, self.final, self.SHAPES, self.tensors = population, single, pheromone, final, SHAPES, tensors
        self._runs = {}

    # ---- the hooks: a net that carries nothing behind the agent state
    def population_kw(self, s, variant):
        """What the population's constructor takes on top of the common arguments."""
        return {}

    def log_extra(self, pop):
        """What a step's log entry holds on top of rot, ph, explored, reward, loss and idx (device copies)."""
        return {}

    def lone(self, s, p, env):
        """Member p's lone trainer and ring, and the state its loop carries from step to step."""
        import torch
        from antsrl_amd import train
        from antsrl_amd.replay import DeviceReplayMemory
        tr = getattr(train, self.single)(F, env.device, discount=s["discount"][p], lr=s["lr"][p], update_target_every=1, seed=s["seed"][p])
        unread = torch.zeros((s["Em"] * s["N"],), dtype=torch.int8, device=env.device)  # without the head, select draws a pheromone that nothing reads
        return tr, DeviceReplayMemory(s["ring"], (7, 7, 6), [2], [2], device=env.device), SimpleNamespace(unread=unread)

    def lone_act(self, s, p, t, tr, env, st, explored, variant):
        """Member p's lone act and select at step t -> rot, ph (None without the head), the memory record_pre takes, the
        one record_post takes, and name -> tensor of what the step's log entry must hold of the member's rows besides."""
        from antsrl_amd import _lib
        rot, ph = tr.policy.act(env.obs, env.agent_state, env=env)
        rot = rot.reshape(-1).clone()
        if self.pheromone:
            ph = ph.reshape(-1).clone()
        else:
            none = ph
            assert none is None
        drawn = ph if self.pheromone else st.unread
        _lib.check(_lib.load().antsrl_agent_select_actions(s["seed"][p], t, p * s["Em"], s["Em"], s["N"], s["epsilon"][p], 3, 3, ptr(rot),
                                                           ptr(drawn), ptr(explored), stream()))
        return rot, ph, None, None, {}

    def same_extra(self, pop, p, tr, st):
        """What same_member compares on top of the ring, the trainers and the counters."""

    def final_of(self, pop):
        """Copies of what the tests read of the run's end besides the counters and the ring's head and fill."""
        return {self.final: getattr(pop.trainer, self.final).clone()}

    # ---- the comparison
    def run_population(self, s, variant=None):
        """s: one of SHAPES.  The population's `steps` rollout_steps under a sync debug mode that makes any read-back an
        error; returns the agent, its environment and per step (device copies) rot, ph, explored, reward, the loss (a
        [P] tensor, or 0), the [P, B] minibatch indices (None while it does not train) and the kind's log_extra."""
        import torch
        from antsrl_amd import population
        whole, shards = make_envs(s["P"], s["Em"], s["N"], s["max_time"], s["bf16"])
        if "slice_bytes" in s:
            assert s["Em"] * s["N"] * F * (2 if s["bf16"] else 4) == s["slice_bytes"] and s["slice_bytes"] % 16 == 0
        assert (s["Em"] * s["N"] * F * (2 if s["bf16"] else 4)) % 16 == 0  # the acting kernel's alignment rule
        pop = getattr(population, self.population)(members_of(s), record_per_step=s["K"], replay_size=s["ring"], minibatch=s["B"],
                                                   min_replay=s["min_replay"], update_target_every=1, seed=3,
                                                   **self.population_kw(s, variant))
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
                                           reward=whole.reward.clone(), loss=loss, idx=pop.trainer.last_idx if trained else None,
                                           **self.log_extra(pop)))
        finally:
            torch.cuda.set_sync_debug_mode(0)
        return SimpleNamespace(pop=pop, env=whole, shards=shards, log=log, variant=variant)

    def run_member_alone(self, s, p, run):
        """Member p alone on its shard handle, entry by entry: the single trainer (seed, lr, discount of the member) and
        its acting policy, the single agent's select (lone_act), record_pre, step_update, record_post (the last three
        without a pheromone for a net that has none, and with the memories lone_act names), then train_on the population's
        own indices once fill >= min_replay.  After every step rot, ph (with that head) and explored of the member's slice,
        what lone_act names besides, env.reward of its rows and loss[p] are equal; returns the member's trainer, ring and
        carried state."""
        import torch
        from antsrl_amd import config as cm
        Em, N = s["Em"], s["N"]
        Mm, env = Em * N, run.shards[p]
        tr, rm, st = self.lone(s, p, env)
        env.set_activation(torch.full((Em, N, env.cfg.n_phero), 10.0, device=env.device))
        env.observe()
        explored = torch.zeros((Em,), dtype=torch.uint8, device=env.device)
        rows, envs = slice(p * Mm, (p + 1) * Mm), slice(p * Em, (p + 1) * Em)
        for t, want in enumerate(run.log):
            obs, ast = env.obs, env.agent_state
            rot, ph, mem_pre, mem_post, extra = self.lone_act(s, p, t, tr, env, st, explored, run.variant)
            assert torch.equal(rot, want.rot[rows]), ("rot", p, t)
            if self.pheromone:
                assert torch.equal(ph, want.ph[rows]), ("ph", p, t)
            assert torch.equal(explored, want.explored[envs]), ("explored", p, t)
            for name, mine in extra.items():
                assert torch.equal(mine, getattr(want, name)[rows]), (name, p, t)
            rm.record_pre(obs, ast, mem_pre, rot, ph, n_envs=Em, n_ants=N, k=s["K"], seed=s["seed"][p], step=t, env_id_base=p * Em)
            done = env.query(cm.Q_TIMESTEP) == s["max_time"]
            env.step_update(rot.view(Em, N), ph.view(Em, N) if self.pheromone else None)
            rm.record_post(env.obs, env.agent_state, mem_post, env.reward.view(-1), env.done)
            assert torch.equal(env.reward.view(-1), want.reward.view(-1)[rows]), ("reward", p, t)
            if rm.fill >= s["min_replay"]:
                assert want.idx is not None, ("the population did not train at step", t)
                loss = tr.train_on(rm, want.idx[p], done)
                assert torch.equal(loss, want.loss[p]), ("loss", p, t, float(loss), float(want.loss[p]))
            else:
                assert want.idx is None and not torch.is_tensor(want.loss) and want.loss == 0, ("the population trained at step", t)
        return tr, rm, st

    def same_trainers(self, t, p, tr):
        """Member p's weights, target, Adam's moments and gradients in the population trainer `t` are the lone trainer
        `tr`'s, and so are the dicts made of them."""
        import torch
        for name, mine, alone in self.tensors(t, p, tr):
            assert torch.equal(mine, alone), (name, p)
        sd, alone_sd = t.state_dict(p), tr.state_dict()
        assert list(sd) == list(alone_sd) and all(torch.equal(sd[k], alone_sd[k]) for k in sd)
        td, alone_td = t.target_state_dict(p), tr.target_state_dict()
        assert list(td) == list(alone_td) and all(torch.equal(td[k], alone_td[k]) for k in td)
        ad, alone_ad = t.adam_state(p), tr.adam_state()
        assert ad["step"] == alone_ad["step"] and all(torch.equal(ad[m][k], alone_ad[m][k]) for m in ("exp_avg", "exp_avg_sq") for k in ad[m])

    def same_member(self, pop, p, tr, rm, st):
        """At the end: all seven ring tensors with head and fill, the weights, the target, Adam's moments, the gradients
        and the counters of member p are its lone run's, and what the kind's same_extra compares."""
        same_rings(pop.replay_memory.member(p), rm)
        t = pop.trainer
        self.same_trainers(t, p, tr)
        assert (t.step_count, t.syncs) == (tr.step_count, tr.syncs), ((t.step_count, t.syncs), (tr.step_count, tr.syncs))
        self.same_extra(pop, p, tr, st)

    def checked_run(self, name, variant=None):
        """The run of SHAPES[name] (in the kind's `variant` when none is given) with every member checked against its lone
        run, once per session, kind, shape and variant (the hand-over test reads the explore shape (b)'s population,
        test_copy_member goes on with shape (a)'s)."""
        key = (name, variant or self.variant)
        if key not in self._runs:
            s = self.SHAPES[name]
            run = self.run_population(s, key[1])
            for p in range(s["P"]):
                self.same_member(run.pop, p, *self.run_member_alone(s, p, run))
            t, ring = run.pop.trainer, run.pop.replay_memory  # as the run left them (test_copy_member goes on with the agent)
            run.final = SimpleNamespace(step_count=t.step_count, syncs=t.syncs, fill=ring.fill, head=ring.head, **self.final_of(run.pop))
            self._runs[key] = run
        return self._runs[key]

    def check_copy_member(self, weights, theirs):
        """copy_member on shape (a)'s population after its comparison.  weights(p) -> copies of member p's weights, target
        and Adam's moments (and whatever else the copy takes along whether or not it takes the ring); theirs: the test's
        words for "these are member 0's"."""
        import torch
        run = self.checked_run("a")
        pop = run.pop
        rm = pop.replay_memory
        slab = lambda p: [getattr(rm, n)[p].clone() for n in RING]  # noqa: E731
        before_w, before_s = [weights(p) for p in range(3)], [slab(p) for p in range(3)]
        assert not all(torch.equal(a, b) for a, b in zip(before_s[0], before_s[2]))
        pop.copy_member(0, 2, ring=False)
        assert all(torch.equal(a, b) for a, b in zip(weights(2), before_w[0])), theirs
        assert all(torch.equal(a, b) for a, b in zip(slab(2), before_s[2])), "with ring=False the slab stays"
        pop.copy_member(0, 2)
        assert all(torch.equal(a, b) for a, b in zip(weights(2), before_w[0]))
        assert all(torch.equal(a, b) for a, b in zip(slab(2), before_s[0])), "the ring slab is member 0's"
        for p in (0, 1):
            assert all(torch.equal(a, b) for a, b in zip(weights(p), before_w[p])), "member %d changed" % p
            assert all(torch.equal(a, b) for a, b in zip(slab(p), before_s[p])), "member %d's slab changed" % p
        assert list(pop.epsilon) == [0.0, 0.5, 1.0]  # the hyper-parameters stay the member's own
        # the population still steps: member 2 now trains member 0's weights on member 0's rows, under its own hyper-parameters
        loss = pop.rollout_step(run.env)
        assert loss.shape == (3,) and bool(torch.isfinite(loss).all())


class MemoryKind(Kind):
    """A population whose net carries a memory: PopulationMemoryAgent against MemoryTrainer, its acting policy with the
    carried memory and antsrl_agent_select.  A shape names the net (power, mem); the variant is the population's
    state_memory.  A step's log entry holds the new memory (`mem`); the lone loop carries the two memory halves."""

    variant = "reference"

    def population_kw(self, s, variant):
        return dict(mem_size=s["mem"], power=s["power"], state_memory=variant)

    def log_extra(self, pop):
        return dict(mem=pop.previous_memory.clone())

    def lone(self, s, p, env):
        import torch
        from antsrl_amd.replay import DeviceReplayMemory
        from antsrl_amd.train import MemoryTrainer
        tr = MemoryTrainer(F, env.device, discount=s["discount"][p], lr=s["lr"][p], update_target_every=1, power=s["power"],
                           mem_size=s["mem"], seed=s["seed"][p])
        halves = [torch.zeros((s["Em"] * s["N"], s["mem"]), device=env.device) for _ in range(2)]
        return tr, DeviceReplayMemory(s["ring"], (7, 7, 6), [2 + s["mem"]], [2], device=env.device), SimpleNamespace(halves=halves, cur=0)

    def lone_act(self, s, p, t, tr, env, st, explored, variant):
        from antsrl_amd import _lib
        old, new = st.halves[st.cur], st.halves[1 - st.cur]
        rot, ph, _ = tr.policy.act(env.obs, env.agent_state, memory=old, out=new, env=env)
        rot, ph = rot.reshape(-1).clone(), ph.reshape(-1).clone()
        _lib.check(_lib.load().antsrl_agent_select(s["seed"][p], t, p * s["Em"], s["Em"], s["N"], s["epsilon"][p], 3, 3, s["mem"], ptr(rot),
                                                   ptr(ph), ptr(old), ptr(new), ptr(explored), stream()), "agent_select")
        st.cur = 1 - st.cur
        return rot, ph, new if variant == "reference" else old, new, dict(mem=new)

    def same_extra(self, pop, p, tr, st):
        """The dict has the reference's 26 tensors; both memory halves, the current one first."""
        import torch
        Mm = pop.g.Mm
        rows = slice(p * Mm, (p + 1) * Mm)
        assert len(pop.trainer.state_dict(p)) == 26
        assert torch.equal(pop._mem[pop._cur][rows], st.halves[st.cur]) and torch.equal(pop._mem[1 - pop._cur][rows], st.halves[1 - st.cur])

    def final_of(self, pop):
        ring = pop.replay_memory
        return dict(model=pop.trainer._model.clone(), agent_states=ring.agent_states.clone(), new_agent_states=ring.new_agent_states.clone())


COLLECT = Kind("PopulationAgent", "LinearTrainer", True, "heads",
               dict(a=dict(_A, slice_bytes=23520), b=dict(_B, B=264, slice_bytes=37632)),
               lambda t, p, tr: (("w1", t.w1[p], tr.policy.w1), ("b1", t.b1[p], tr.policy.b1), ("heads", t.heads[p], tr.heads),
                                 ("target_l3", t.target_l3[p], tr.target_l3), ("adam", t._adam[p], tr._adam),
                                 ("grads", t.grads[p], tr.grads)))
EXPLORE = Kind("PopulationExploreAgent", "ExploreTrainer", False, "model", dict(a=_A, b=dict(_B, B=136)),
               lambda t, p, tr: (("model", t.model[p], tr.model), ("target", t.target[p], tr.target),
                                 ("adam m", t._adam[0, p], tr._adam[0]), ("adam v", t._adam[1, p], tr._adam[1]),
                                 ("grads", t.grads[p], tr.grads)))
#: (a) is _A with a small net; (b) is _B with the reference's B = 264, power 5 and mem 20.  The state blocks hold the
#: masters, Adam's moments and the training packs: compared byte for byte, with the acting pack
MEMORY = MemoryKind("PopulationMemoryAgent", "MemoryTrainer", True, "_model",
                    dict(a=dict(_A, power=4, mem=3), b=dict(_B, B=264, power=5, mem=20)),
                    lambda t, p, tr: (("the model's state block", t._model[p], tr._model), ("the target's state block", t._target[p], tr._target),
                                      ("the acting pack", t.packed[p], tr.policy.packed), ("grads", t.grads[p], tr.grads)))
