"""What the device tests of the agents share (test_gpu_linear_agent.py, test_gpu_explore_agent.py, test_gpu_memory_agent.py,
test_gpu_memory_agent_skip.py): pointers for the C entries, the small environment they all act in, the
comparison of two replay rings, the tolerance of an Adam step's parameters, and the two loop comparisons every in-loop
agent is held to, an agent's fused loop against the same loop driven entry by entry from the host (drive_loop) and its
in-loop acting against its standalone acting (inloop_runs).  A test file keeps its agent, its trainer and the assertions
that are its agent's own.  torch is imported inside the functions, as in the GPU test files."""
import ctypes as C
from types import SimpleNamespace

from dqn_ref import RING


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_rings(a, b, names=RING):
    import torch
    for n in names:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert (a.head, a.fill) == (b.head, b.fill), ((a.head, a.fill), (b.head, b.fill))


def make_env(E=4, N=64, max_time=2000, seed=5, dtype=None, meta=False):
    """E colonies of N ants on 64 x 64 cells with 7 x 7 x 6 observations; meta: the cell-meta step path, which the
    in-loop policy needs."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    kw = dict(act_path=cm.ACT_CELL_META) if meta else {}
    cfg = cm.make_cfg(E, N, 64, 64, deposit_strength=256.0, max_time=max_time, **kw)
    env = BatchedAntsEnv(cfg, obs_dtype=dtype or torch.float32)
    env.reset(synth_init(cfg, seed=seed, n_food_discs=6, food_rmin=3, food_rmax=6))
    return env


def param_tolerance(ref_after, before):
    """Device and torch evaluate the same fp32 expression p + -step_size * (m / denom) from bit-equal m and v; they may
    round the update term differently by an ulp or two of the UPDATE, and the sum then lands on a neighbouring float:
    one ulp of the parameter, 2^-23 |p|, plus 4 ulps of the update itself for parameters smaller than their update."""
    return 2.0 ** -23 * (ref_after.abs() + 4 * (ref_after - before).abs())


def _acted(agent, pheromone):
    """What the step acted with (device copies: no read-back)."""
    return (agent._rot.clone(), agent._ph.clone()) if pheromone else (agent._rot.clone(),)


def drive_loop(agent, trainer_cls, minibatch, pheromone, synced, steps, E=4, N=64, max_time=12):
    """`steps` rollout_steps of `agent`'s fused loop, under a sync debug mode that makes any read-back an error, and the
    same loop driven from the host one entry at a time: trainer_cls's policy, antsrl_agent_select_actions, record_pre,
    step_update, record_post, train(minibatch).  The agent is one built with epsilon 0.5, learning rate 1e-3, min_replay
    500, a 3000-row ring and seed 7.  pheromone: whether a pheromone action goes to select_actions, record_pre and
    step_update (else NULL, a scratch buffer for the entry that needs a pointer).  synced(trainer): is the target equal
    to the model?  It is asked after every training step that ends an episode.

    Returns losses / host_losses and acts / host_acts per step (acts: (rotation, pheromone) or (rotation,)), the host's
    trainer and ring, synced_after_done, both environments and the activation set before the host's first step."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.replay import DeviceReplayMemory
    lib = _lib.load()
    env_a, env_b = make_env(E, N, max_time), make_env(E, N, max_time)
    agent.setup(env_a)
    agent.initialize(env_a)
    env_a.observe()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # the fused loop reads nothing back
    losses, acts = [], []
    try:
        for t in range(steps):
            losses.append(agent.rollout_step(env_a))
            acts.append(_acted(agent, pheromone))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    # ---- the same loop, host-driven, one entry at a time
    M, F = E * N, 294
    tr = trainer_cls(F, env_b.device, lr=1e-3, seed=7)
    rm = DeviceReplayMemory(3000, (7, 7, 6), [2], [2], device=env_b.device)
    gen = torch.Generator(device=env_b.device)
    gen.manual_seed(7)
    activation = torch.full((E, N, 2), 10.0, device=env_b.device)
    env_b.set_activation(activation)
    obs, ast, _ = env_b.observe()
    scratch = None if pheromone else torch.zeros((M,), dtype=torch.int8, device="cuda")
    host_losses, host_acts, synced_after_done = [], [], []
    for t in range(steps):
        rot, ph = tr.policy.act(obs, ast)
        rot, ph = rot.reshape(-1).clone(), (ph.reshape(-1).clone() if pheromone else None)
        _lib.check(lib.antsrl_agent_select_actions(7, t, 0, E, N, 0.5, 3, 3, ptr(rot), ptr(ph if pheromone else scratch), None,
                                                   stream()))
        host_acts.append((rot, ph) if pheromone else (rot,))
        rm.record_pre(obs, ast, None, rot, ph, n_envs=E, n_ants=N, seed=7, step=t)
        done = env_b.query(cm.Q_TIMESTEP) == max_time
        env_b.step_update(rot.view(E, N), ph.view(E, N) if pheromone else None)
        rm.record_post(env_b.obs, env_b.agent_state, None, env_b.reward.view(-1), env_b.done)
        host_losses.append(tr.train(rm, done, minibatch=minibatch, min_replay=500, generator=gen))
        if done and tr.step_count:
            synced_after_done.append(synced(tr))
    return SimpleNamespace(losses=losses, host_losses=host_losses, acts=acts, host_acts=host_acts, trainer=tr, ring=rm,
                           synced_after_done=synced_after_done, env_a=env_a, env_b=env_b, activation=activation)


def inloop_runs(make_agent, pheromone, steps, E=4, N=64, max_time=12):
    """The same `steps` rollout_steps with standalone and with in-loop acting, on bfloat16 observations and the cell-meta
    path: make_agent(inloop=..., record_per_step=50) builds the agent (50 rows per step: the first steps stay below
    min_replay and do not train).  Returns the two runs, standalone first: agent, env, acts and losses per step, and
    after_sync, the number of steps that were the first after a sync of the target (the last step's sync is followed by
    none)."""
    import torch
    runs = []
    for inloop in (False, True):
        env = make_env(E, N, max_time, dtype=torch.bfloat16, meta=True)
        ag = make_agent(inloop=inloop, record_per_step=50)
        ag.setup(env)
        ag.initialize(env)
        env.observe()
        acts, losses, after_sync = [], [], 0
        for t in range(steps):
            v = ag.trainer.version
            losses.append(ag.rollout_step(env))
            acts.append(_acted(ag, pheromone))
            after_sync += int(t + 1 < steps and ag.trainer.version != v)  # the next step is the first after a sync
        runs.append(SimpleNamespace(agent=ag, env=env, acts=acts, losses=losses, after_sync=after_sync))
    return runs
