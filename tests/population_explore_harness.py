"""What the device tests of the explore population share (test_gpu_population_explore.py): the two shapes of the
acceptance test and the comparison itself — a PopulationExploreAgent's fused loop against every member run ALONE on a
shard handle of its own environments, driven entry by entry (ExploreTrainer, its LinearPolicy without a pheromone head,
antsrl_agent_select_actions, DeviceReplayMemory), as population_harness.run_member_alone does for the linear agent.  The
environments are population_harness.make_envs'.  torch is imported inside the functions, as in the GPU test files."""
from types import SimpleNamespace

from agent_harness import ptr, same_rings, stream
from population_harness import F, make_envs, members_of

#: the acceptance test's two shapes.  (a): 40 ants per member (a whole tile and one of 8 rows), bfloat16 on the cell-meta
#: path; members 0 and 2 share a seed and must still differ through their environment ids; B = 48 is one whole tile and
#: half of one, in ONE forward workgroup; 40 rows per step wrap the 200-row ring in step 5.  (b): float32, K = 24 (the
#: stratified sample) wraps the 300-row ring at step 13; B = 136 is five tiles, so a member has TWO forward workgroups, the
#: second with one tile of 8 valid rows, and the layer1 stage adds their partials in workgroup order.  max_time 8 gives
#: an episode end and a target sync inside either run.
SHAPES = dict(
    a=dict(P=3, Em=2, N=20, bf16=True, epsilon=(0.0, 0.5, 1.0), lr=(1e-3, 1e-4, 3e-3), discount=(0.5, 0.99, 0.9),
           seed=(7, 8, 7), K=None, ring=200, min_replay=80, B=48, max_time=8, steps=14),
    b=dict(P=2, Em=1, N=32, bf16=False, epsilon=(0.5, 0.5), lr=(1e-3, 1e-3), discount=(0.5, 0.99), seed=(7, 9), K=24,
           ring=300, min_replay=48, B=136, max_time=8, steps=18),
)


def run_population(s):
    """s: one of SHAPES.  The population's `steps` rollout_steps under a sync debug mode that makes any read-back an
    error; returns the agent, its environment and per step (device copies) rot, explored, reward, the loss (a [P] tensor,
    or 0) and the [P, B] minibatch indices (None while it does not train)."""
    import torch
    from antsrl_amd.population import PopulationExploreAgent
    whole, shards = make_envs(s["P"], s["Em"], s["N"], s["max_time"], s["bf16"])
    assert (s["Em"] * s["N"] * F * (2 if s["bf16"] else 4)) % 16 == 0  # the acting kernel's alignment rule
    pop = PopulationExploreAgent(members_of(s), record_per_step=s["K"], replay_size=s["ring"], minibatch=s["B"],
                                 min_replay=s["min_replay"], update_target_every=1, seed=3)
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
            log.append(SimpleNamespace(rot=pop._rot.clone(), explored=pop._explored.clone(), reward=whole.reward.clone(),
                                       loss=loss, idx=pop.trainer.last_idx if trained else None))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return SimpleNamespace(pop=pop, env=whole, shards=shards, log=log)


def run_member_alone(s, p, run):
    """Member p alone on its shard handle, entry by entry: ExploreTrainer(seed, lr, discount of the member) and its acting
    policy (the target block), antsrl_agent_select_actions, record_pre without a pheromone, step_update without one,
    record_post, then train_on the population's own indices once fill >= min_replay.  After every step rot and explored
    of the member's slice, env.reward of its rows and loss[p] are equal; returns the member's trainer and ring."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.replay import DeviceReplayMemory
    from antsrl_amd.train import ExploreTrainer
    lib = _lib.load()
    Em, N = s["Em"], s["N"]
    Mm, env = Em * N, run.shards[p]
    seed, eps = s["seed"][p], s["epsilon"][p]
    tr = ExploreTrainer(F, env.device, discount=s["discount"][p], lr=s["lr"][p], update_target_every=1, seed=seed)
    rm = DeviceReplayMemory(s["ring"], (7, 7, 6), [2], [2], device=env.device)
    env.set_activation(torch.full((Em, N, env.cfg.n_phero), 10.0, device=env.device))
    env.observe()
    explored = torch.zeros((Em,), dtype=torch.uint8, device=env.device)
    ph = torch.zeros((Mm,), dtype=torch.int8, device=env.device)  # select draws a pheromone that nothing reads
    rows, envs = slice(p * Mm, (p + 1) * Mm), slice(p * Em, (p + 1) * Em)
    for t, want in enumerate(run.log):
        obs, ast = env.obs, env.agent_state
        rot, none = tr.policy.act(obs, ast, env=env)
        assert none is None
        rot = rot.reshape(-1).clone()
        _lib.check(lib.antsrl_agent_select_actions(seed, t, p * Em, Em, N, eps, 3, 3, ptr(rot), ptr(ph), ptr(explored), stream()))
        assert torch.equal(rot, want.rot[rows]), ("rot", p, t)
        assert torch.equal(explored, want.explored[envs]), ("explored", p, t)
        rm.record_pre(obs, ast, None, rot, None, n_envs=Em, n_ants=N, k=s["K"], seed=seed, step=t, env_id_base=p * Em)
        done = env.query(cm.Q_TIMESTEP) == s["max_time"]
        env.step_update(rot.view(Em, N), None)
        rm.record_post(env.obs, env.agent_state, None, env.reward.view(-1), env.done)
        assert torch.equal(env.reward.view(-1), want.reward.view(-1)[rows]), ("reward", p, t)
        if rm.fill >= s["min_replay"]:
            assert want.idx is not None, ("the population did not train at step", t)
            loss = tr.train_on(rm, want.idx[p], done)
            assert torch.equal(loss, want.loss[p]), ("loss", p, t, float(loss), float(want.loss[p]))
        else:
            assert want.idx is None and not torch.is_tensor(want.loss) and want.loss == 0, ("the population trained at step", t)
    return tr, rm


def same_trainers(t, p, tr):
    """Member p's model and target blocks, Adam's moments and gradients in the population trainer `t` are ExploreTrainer
    `tr`'s, and so are the dicts made of them."""
    import torch
    for name, mine, alone in (("model", t.model[p], tr.model), ("target", t.target[p], tr.target),
                              ("adam m", t._adam[0, p], tr._adam[0]), ("adam v", t._adam[1, p], tr._adam[1]),
                              ("grads", t.grads[p], tr.grads)):
        assert torch.equal(mine, alone), (name, p)
    sd, alone_sd = t.state_dict(p), tr.state_dict()
    assert list(sd) == list(alone_sd) and all(torch.equal(sd[k], alone_sd[k]) for k in sd)
    td, alone_td = t.target_state_dict(p), tr.target_state_dict()
    assert list(td) == list(alone_td) and all(torch.equal(td[k], alone_td[k]) for k in td)
    ad, alone_ad = t.adam_state(p), tr.adam_state()
    assert ad["step"] == alone_ad["step"] and all(torch.equal(ad[m][k], alone_ad[m][k]) for m in ("exp_avg", "exp_avg_sq") for k in ad[m])


def same_member(pop, p, tr, rm):
    """At the end: all seven ring tensors with head and fill, the model and target blocks, Adam's moments, the gradients
    and the counters of member p are its lone run's."""
    same_rings(pop.replay_memory.member(p), rm)
    t = pop.trainer
    same_trainers(t, p, tr)
    assert (t.step_count, t.syncs) == (tr.step_count, tr.syncs), ((t.step_count, t.syncs), (tr.step_count, tr.syncs))


_RUNS = {}


def checked_run(name):
    """The run of SHAPES[name] with every member checked against its lone run, once per session (the hand-over test reads
    shape (b)'s population, test_copy_member goes on with shape (a)'s)."""
    if name not in _RUNS:
        s = SHAPES[name]
        run = run_population(s)
        for p in range(s["P"]):
            tr, rm = run_member_alone(s, p, run)
            same_member(run.pop, p, tr, rm)
        t, ring = run.pop.trainer, run.pop.replay_memory  # as the run left them
        run.final = SimpleNamespace(model=t.model.clone(), step_count=t.step_count, syncs=t.syncs, fill=ring.fill, head=ring.head)
        _RUNS[name] = run
    return _RUNS[name]
