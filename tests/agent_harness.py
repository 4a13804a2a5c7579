"""What the device tests of the agents share (test_gpu_linear_agent.py, test_gpu_explore_agent.py, test_gpu_memory_agent.py,
test_gpu_memory_agent_skip.py): pointers for the C entries, the small environment they all act in, the
comparison of two replay rings, the tolerance of an Adam step's parameters, and the two loop comparisons every in-loop
agent is held to, an agent's fused loop against the same loop driven entry by entry from the host (drive_loop) and its
in-loop acting against its standalone acting (inloop_runs); and for two trainers that must hold equal bits, what a
LinearTrainer or an ExploreTrainer holds after a step, its workspace read back (linear_snapshot, explore_snapshot), and
where two of them differ (twin_report: the localisation of DESIGN §7.13).  A test file keeps its agent, its trainer and the assertions
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


def random_linear_replay(N, F, seed, with_done):
    """A replay of N random rows on the device for the linear trainer (sparse observations, agent states in [-2, 2),
    normal rewards, 30 % dones or none) and the generator it came from, for the indices."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    st, nst = (torch.rand((N, F), device="cuda", generator=g) for _ in range(2))
    st[torch.rand((N, F), device="cuda", generator=g) < 0.5] = 0.0  # observations are sparse
    ast, nast = (torch.rand((N, 2), device="cuda", generator=g) * 4 - 2 for _ in range(2))
    act = torch.randint(0, 3, (N, 2), device="cuda", generator=g)
    rw = torch.randn((N,), device="cuda", generator=g)
    dn = (torch.rand((N,), device="cuda", generator=g) < 0.3) if with_done else torch.zeros((N,), dtype=torch.bool, device="cuda")
    return (st, ast, act, rw, nst, nast, dn), g


# ---- two trainers that must hold equal bits: what differs, for an assertion's message ----------------------------------
def same_bits(a, b):
    """Equal shapes and equal bit patterns (NaN equals the same NaN, -0 is not +0)."""
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ulp_distance(a, b):
    """Per element, how many fp32 values lie between a and b: the distance of the bit patterns on the ordered line."""
    import torch

    def line(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (line(a) - line(b)).abs()


def difference_report(what, ref, got, limit=6, whole_rows=3):
    """"" where ref and got (fp32, on the CPU) hold equal bits; else how many elements differ, over which rows and
    columns of a 2-d tensor, the first `limit` of them (index, both values, the distance in ulps), and per differing row
    how many columns differ and by how much of the row's largest value; the first `whole_rows` differing rows of a 2-d
    tensor follow in full, both sides, nine digits each (enough to restore the fp32)."""
    import torch
    if same_bits(ref, got):
        return ""
    two_d = ref.dim() == 2
    ref, got = ref.reshape(ref.shape if two_d else (1, -1)), got.reshape(got.shape if two_d else (1, -1))
    bad = (ref.contiguous().view(torch.int32) != got.contiguous().view(torch.int32)).nonzero()
    ulps = ulp_distance(ref, got)
    rows, cols = sorted(set(bad[:, 0].tolist())), sorted(set(bad[:, 1].tolist()))
    lines = ["%s: %d of %d differ, worst %d ulp" % (what, len(bad), ref.numel(), int(ulps.max()))]
    lines.append("  first: " + "; ".join("[%d][%d] %.9g against %.9g (%d ulp)" % (r, c, float(ref[r, c]), float(got[r, c]), int(ulps[r, c]))
                                        for r, c in bad[:limit].tolist()))
    if two_d:
        lines.append("  %d rows %s, %d columns %s" % (len(rows), rows[:40] + (["..."] if len(rows) > 40 else []), len(cols),
                                                      cols if len(cols) <= 24 else cols[:24] + ["..."]))
        for r in rows[:12]:
            diff = (ref[r].double() - got[r].double()).abs()
            lines.append("  row %d: %d columns differ, worst %d ulp, largest |difference| %.3g of the row's largest |value| %.3g"
                         % (r, int((ulps[r] > 0).sum()), int(ulps[r].max()), float(diff.max() / ref[r].abs().max()), float(ref[r].abs().max())))
        for r in rows[:whole_rows]:
            lines.append("  row %d, first: %s" % (r, " ".join("%.9g" % v for v in ref[r].tolist())))
            lines.append("  row %d, twin:  %s" % (r, " ".join("%.9g" % v for v in got[r].tolist())))
    return "\n".join(lines)


def twin_report(first, twin, whole_rows=1):
    """first, twin: {quantity: fp32 tensor on the CPU}, with the workgroups' partials under "partials" ([workgroup][output])
    and, under "finish_ok", whether the ordered fp32 sum of a trainer's own partials gives its own gradients and loss.
    One line per quantity that differs: that is the localisation (one workgroup or many, the loss column only or the
    gradients too, the gradient stage or the finish).  Only the partials' first `whole_rows` differing rows are written out whole."""
    lines = [difference_report(k, first[k], twin[k], whole_rows=whole_rows if k == "partials" else 0)
             for k in first if k != "finish_ok" and k in twin]
    lines = [s for s in lines if s]
    if "finish_ok" in first:
        lines.append("the ordered sum of its own partials gives its own gradients and loss: first %s, twin %s"
                     % (first["finish_ok"], twin["finish_ok"]))
    return "\n" + "\n".join(lines)


def linear_snapshot(tr, loss, B, grads=True):
    """What a LinearTrainer holds after a step on B rows (more than 512: the workspace is in use), on the CPU: loss [1],
    heads, adam, the partials [workgroups][199] and, where the step kept them, grads."""
    import torch
    import linear_train_ref as L
    nb = L.blocks(B)
    part = tr._work.cpu().view(torch.float32)[: nb * L.PART].view(nb, L.PART)[:, :L.OUT].clone()
    s = dict(loss=loss.detach().cpu().reshape(1), partials=part, heads=tr.heads.cpu(), adam=tr._adam.cpu())
    total = L.ordered_sum(part)
    s["finish_ok"] = same_bits(total[198:199], s["loss"])
    if grads:
        s["grads"] = tr.grads.cpu()
        s["finish_ok"] = s["finish_ok"] and same_bits(total[:198], s["grads"])
    return s


def explore_snapshot(tr, loss, B, grads=True):
    """The same for an ExploreTrainer: loss [1], model, adam, the partials [workgroups][100], dh [B][32] and grads."""
    import torch
    import explore_train_ref as X
    W = X.work_layout(B)
    work = tr._work.cpu()
    part = work[: W["blocks"] * X.PART * 4].view(torch.float32).view(W["blocks"], X.PART)[:, :X.OUT].clone()
    dh = work[W["dh_offset"]: W["bytes"]].view(torch.float32).view(B, 32).clone()
    s = dict(loss=loss.detach().cpu().reshape(1), partials=part, dh=dh, model=tr.model.cpu(), adam=tr._adam.cpu())
    total = X.ordered_sum(part)
    s["finish_ok"] = same_bits(total[99:100], s["loss"])
    if grads:
        s["grads"] = tr.grads.cpu()
        l2 = 32 * (tr.n_features + 2) + 32
        s["finish_ok"] = s["finish_ok"] and same_bits(total[:99], s["grads"][l2: l2 + 99])
    return s
