"""What the device tests of the population share (test_gpu_population.py): the two shapes of the acceptance test, the
environment a population acts in with the shard handles of its members, and the comparison itself — a PopulationAgent's
fused loop against every member run ALONE on a shard handle of its own environments, driven entry by entry as
agent_harness.drive_loop drives an agent.  torch is imported inside the functions, as in the GPU test files."""
from types import SimpleNamespace

import numpy as np

from agent_harness import ptr, same_rings, stream

F = 294  # 7 x 7 x 6 observations

#: the acceptance test's two shapes.  (a): 40 ants per member, so its second tile has 8 rows; members 0 and 2 share a seed
#: and must still differ through their environment ids; B = 48 is one whole tile and half of one; 40 rows per step wrap
#: the 200-row ring in step 5.  (b): B = 264 is the reference's nine tiles; K = 24 is the stratified sample, and 24 rows
#: per step wrap the 300-row ring at step 13.  max_time 8 gives an episode end and a target sync inside either run.
SHAPES = dict(
    a=dict(P=3, Em=2, N=20, bf16=True, epsilon=(0.0, 0.5, 1.0), lr=(1e-3, 1e-4, 3e-3), discount=(0.5, 0.99, 0.9),
           seed=(7, 8, 7), K=None, ring=200, min_replay=80, B=48, max_time=8, steps=14, slice_bytes=23520),
    b=dict(P=2, Em=1, N=32, bf16=False, epsilon=(0.5, 0.5), lr=(1e-3, 1e-3), discount=(0.5, 0.99), seed=(7, 9), K=24,
           ring=300, min_replay=48, B=264, max_time=8, steps=18, slice_bytes=37632),
)


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


def run_population(s):
    """s: one of SHAPES.  The population's `steps` rollout_steps under a sync debug mode that makes any read-back an
    error; returns the agent, its environment and per step (device copies) rot, ph, explored, reward, the loss (a [P]
    tensor, or 0) and the [P, B] minibatch indices (None while it does not train)."""
    import torch
    from antsrl_amd.population import PopulationAgent
    whole, shards = make_envs(s["P"], s["Em"], s["N"], s["max_time"], s["bf16"])
    assert s["Em"] * s["N"] * F * (2 if s["bf16"] else 4) == s["slice_bytes"] and s["slice_bytes"] % 16 == 0
    pop = PopulationAgent(members_of(s), record_per_step=s["K"], replay_size=s["ring"], minibatch=s["B"],
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
            log.append(SimpleNamespace(rot=pop._rot.clone(), ph=pop._ph.clone(), explored=pop._explored.clone(),
                                       reward=whole.reward.clone(), loss=loss, idx=pop.trainer.last_idx if trained else None))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    return SimpleNamespace(pop=pop, env=whole, shards=shards, log=log)


def run_member_alone(s, p, run):
    """Member p alone on its shard handle, entry by entry: LinearTrainer(seed, lr, discount of the member),
    antsrl_agent_select_actions, record_pre, step_update, record_post, then train_on the population's own indices once
    fill >= min_replay.  After every step rot, ph and explored of the member's slice, env.reward of its rows and loss[p]
    are equal; returns the member's trainer and ring."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.replay import DeviceReplayMemory
    from antsrl_amd.train import LinearTrainer
    lib = _lib.load()
    Em, N = s["Em"], s["N"]
    Mm, env = Em * N, run.shards[p]
    seed, eps = s["seed"][p], s["epsilon"][p]
    tr = LinearTrainer(F, env.device, discount=s["discount"][p], lr=s["lr"][p], update_target_every=1, seed=seed)
    rm = DeviceReplayMemory(s["ring"], (7, 7, 6), [2], [2], device=env.device)
    env.set_activation(torch.full((Em, N, env.cfg.n_phero), 10.0, device=env.device))
    env.observe()
    explored = torch.zeros((Em,), dtype=torch.uint8, device=env.device)
    rows, envs = slice(p * Mm, (p + 1) * Mm), slice(p * Em, (p + 1) * Em)
    for t, want in enumerate(run.log):
        obs, ast = env.obs, env.agent_state
        rot, ph = tr.policy.act(obs, ast, env=env)
        rot, ph = rot.reshape(-1).clone(), ph.reshape(-1).clone()
        _lib.check(lib.antsrl_agent_select_actions(seed, t, p * Em, Em, N, eps, 3, 3, ptr(rot), ptr(ph), ptr(explored), stream()))
        assert torch.equal(rot, want.rot[rows]), ("rot", p, t)
        assert torch.equal(ph, want.ph[rows]), ("ph", p, t)
        assert torch.equal(explored, want.explored[envs]), ("explored", p, t)
        rm.record_pre(obs, ast, None, rot, ph, n_envs=Em, n_ants=N, k=s["K"], seed=seed, step=t, env_id_base=p * Em)
        done = env.query(cm.Q_TIMESTEP) == s["max_time"]
        env.step_update(rot.view(Em, N), ph.view(Em, N))
        rm.record_post(env.obs, env.agent_state, None, env.reward.view(-1), env.done)
        assert torch.equal(env.reward.view(-1), want.reward.view(-1)[rows]), ("reward", p, t)
        if rm.fill >= s["min_replay"]:
            assert want.idx is not None, ("the population did not train at step", t)
            loss = tr.train_on(rm, want.idx[p], done)
            assert torch.equal(loss, want.loss[p]), ("loss", p, t, float(loss), float(want.loss[p]))
        else:
            assert want.idx is None and not torch.is_tensor(want.loss) and want.loss == 0, ("the population trained at step", t)
    return tr, rm


def same_member(pop, p, tr, rm):
    """At the end: all seven ring tensors with head and fill, heads, target_l3, Adam's moments, the gradients and the step
    count of member p are its lone run's."""
    import torch
    same_rings(pop.replay_memory.member(p), rm)
    t = pop.trainer
    for name, mine, alone in (("w1", t.w1[p], tr.policy.w1), ("b1", t.b1[p], tr.policy.b1), ("heads", t.heads[p], tr.heads),
                              ("target_l3", t.target_l3[p], tr.target_l3), ("adam", t._adam[p], tr._adam),
                              ("grads", t.grads[p], tr.grads)):
        assert torch.equal(mine, alone), (name, p)
    assert (t.step_count, t.syncs) == (tr.step_count, tr.syncs), ((t.step_count, t.syncs), (tr.step_count, tr.syncs))
    sd, alone_sd = t.state_dict(p), tr.state_dict()
    assert list(sd) == list(alone_sd) and all(torch.equal(sd[k], alone_sd[k]) for k in sd)
    td, alone_td = t.target_state_dict(p), tr.target_state_dict()
    assert all(torch.equal(td[k], alone_td[k]) for k in td)
    ad, alone_ad = t.adam_state(p), tr.adam_state()
    assert ad["step"] == alone_ad["step"] and all(torch.equal(ad[m][k], alone_ad[m][k]) for m in ("exp_avg", "exp_avg_sq") for k in ad[m])


_RUNS = {}


def checked_run(name):
    """The run of SHAPES[name] with every member checked against its lone run, once per session (test_copy_member works on
    shape (a)'s population after the comparison has been made)."""
    if name not in _RUNS:
        s = SHAPES[name]
        run = run_population(s)
        for p in range(s["P"]):
            tr, rm = run_member_alone(s, p, run)
            same_member(run.pop, p, tr, rm)
        t, ring = run.pop.trainer, run.pop.replay_memory  # as the run left them (test_copy_member goes on with the agent)
        run.final = SimpleNamespace(heads=t.heads.clone(), step_count=t.step_count, syncs=t.syncs, fill=ring.fill, head=ring.head)
        _RUNS[name] = run
    return _RUNS[name]
