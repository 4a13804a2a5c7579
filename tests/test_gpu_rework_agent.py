"""The rework agent on the device: antsrl_policy_rework_select (the forward pass and the epsilon-greedy select in one
launch) and ReworkAgent on _DeviceAgent's loop.

Every comparison is bit for bit but the last test's, which is a monotone statement:
  1  the fused entry's rotation, pheromone and explored against antsrl_policy_rework + antsrl_agent_select_actions,
     against memory_agent_ref.select (the header's draw specification in numpy) on the device's own argmaxes, and
     against a second launch of itself
  2  an exploring colony's observation and agent-state rows do not matter (NaN over them changes nothing)
  3  q_out: antsrl_policy_rework's bits on the rows of the colonies that do not explore, untouched elsewhere
  4  nothing outside rotation, pheromone, explored and q_out is written
  5  ReworkAgent acts like the reference on the fixture's recorded steps
  6  rollout_step equals the same loop driven entry by entry (agent_harness.drive_loop: float32, one episode end; and a
     loop of the same form here: both formats, two episode ends)
  7  save_model / load_model
  8  the loss falls on one minibatch
The GPU tests read only the fixtures, never the reference's checkout."""
import functools

import numpy as np
import pytest

import memory_agent_ref as A
import rework_policy_ref as R
from agent_harness import drive_loop, make_env, same_bits, same_rings

pytestmark = pytest.mark.gpu

FORMATS = ("float32", "bfloat16")
SHAPES = ((4, 64), (7, 33), (5, 17), (3, 1), (1, 1), (9, 8), (6, 7), (16, 512))  # (colonies, ants per colony)
#: a wave pass is eight rows: (7, 33) and (6, 7) have passes that straddle colonies, (16, 512) has none
AXES = ((7, 33), (6, 7), (16, 512))
ROWS = 16 * 512
BASE = dict(F=294, heads=(3, 3), fmt="float32", eps=0.5, base=0, step=1)
PATTERN = 0x5AA55AA5  # q_out's prefill


def _cases():
    """Every shape at the base setting in both formats; every other axis against AXES."""
    out = [dict(BASE, EN=en, fmt=f) for en in SHAPES for f in FORMATS]
    for en in AXES:
        out += [dict(BASE, EN=en, F=F, fmt=f) for F in (9, 62, 1022) for f in FORMATS]  # F = 9: odd bfloat16 rows
        out += [dict(BASE, EN=en, F=62, heads=h, fmt=f) for h in ((1, 8), (2, 5)) for f in FORMATS]
        out += [dict(BASE, EN=en, eps=e, fmt=f) for e, f in ((0.0, "float32"), (0.1, "bfloat16"), (1.0, "float32"), (1.0, "bfloat16"))]
        out += [dict(BASE, EN=en, base=b) for b in (3, 1 << 20)]
        out += [dict(BASE, EN=en, step=123456789)]
    return out


def _id(c):
    return "E%dxN%d-F%d-h%d+%d-%s-eps%g-base%d-step%d" % (c["EN"] + (c["F"],) + c["heads"] + (c["fmt"], c["eps"], c["base"], c["step"]))


@functools.lru_cache(maxsize=None)
def _net(F, heads):
    """(policy, obs [ROWS, F], agent_state [ROWS, 2]) on the CPU but for the policy: rework_policy_ref's synthetic recipe,
    whose values are bfloat16 values, so both formats carry equal inputs."""
    from antsrl_amd.policy import ReworkPolicy
    sd, obs, ast = R.synthetic(F, heads[0], heads[1], ROWS, 1)
    pol = ReworkPolicy(F, "cuda", seed=99)
    pol.load_state_dict(sd)
    return pol, obs, ast


def _seeds(E, eps, base, step):
    """Seeds under which the restatement has an exploring and a non-exploring colony: one seed, or for a single colony
    two, one of each kind.  Epsilon 0 and 1 have one kind only."""
    if eps in (0.0, 1.0):
        return [1]
    ex = {s: A.explores(s, step, base, E, eps) for s in range(1, 400)}
    if E == 1:
        seeds = [next(s for s, e in ex.items() if e[0]), next(s for s, e in ex.items() if not e[0])]
        assert ex[seeds[0]].all() and not ex[seeds[1]].any()
        return seeds
    s = next(s for s, e in ex.items() if e.any() and not e.all())
    assert 0 < int(ex[s].sum()) < E
    return [s]


class _Run:
    """One case's inputs on the device and its launches."""

    def __init__(self, c):
        import torch
        self.c, (self.E, self.N) = c, c["EN"]
        self.M = self.E * self.N
        self.pol, obs, ast = _net(c["F"], c["heads"])
        self.NQ = sum(c["heads"])
        self.obs = obs[:self.M].to("cuda", getattr(torch, c["fmt"])).view(self.E, self.N, 1, 1, c["F"]).contiguous()
        self.ast = ast[:self.M].to("cuda").view(self.E, self.N, 2).contiguous()

    def _out(self):
        import torch
        return (torch.full((self.M,), 99, dtype=torch.int8, device="cuda"), torch.full((self.M,), 99, dtype=torch.int8, device="cuda"),
                torch.full((self.E,), 99, dtype=torch.uint8, device="cuda"))

    def fused(self, seed, obs=None, ast=None, logits=None):
        rot, ph, ex = self._out()
        c = self.c
        self.pol.act_select(self.obs if obs is None else obs, self.ast if ast is None else ast, seed=seed, step=c["step"],
                            env_id_base=c["base"], n_envs=self.E, n_ants=self.N, epsilon=c["eps"], out=(rot, ph), explored=ex,
                            logits=logits)
        return rot.cpu(), ph.cpu(), ex.cpu()

    def two_launches(self, seed, logits=None):
        """-> (the argmaxes, what antsrl_agent_select_actions leaves of them and explored)."""
        from antsrl_amd import _lib
        from agent_harness import ptr, stream
        rot, ph, ex = self._out()
        c = self.c
        self.pol.act(self.obs, self.ast, out=(rot, ph), logits=logits)
        greedy = rot.cpu(), ph.cpu()
        _lib.check(_lib.load().antsrl_agent_select_actions(seed, c["step"], c["base"], self.E, self.N, c["eps"], c["heads"][0],
                                                           c["heads"][1], ptr(rot), ptr(ph), ptr(ex), stream()))
        return greedy, (rot.cpu(), ph.cpu(), ex.cpu())

    def restated(self, seed, greedy):
        import torch
        c, z = self.c, np.zeros((self.E, self.N, 1), dtype=np.float32)
        rot, ph, _, ex = A.select(seed, c["step"], c["base"], c["eps"], c["heads"][0], c["heads"][1],
                                  greedy[0].numpy().reshape(self.E, self.N), greedy[1].numpy().reshape(self.E, self.N), z, z)
        return torch.from_numpy(rot.reshape(-1)), torch.from_numpy(ph.reshape(-1)), torch.from_numpy(ex.astype(np.uint8))


def _equal(a, b, what):
    import torch
    for x, y, n in zip(a, b, ("rotation", "pheromone", "explored")):
        assert x.dtype == y.dtype and torch.equal(x, y), "%s: %s differs at %s" % (what, n, (x != y).nonzero().view(-1)[:8].tolist())


# ---- 1
@pytest.mark.parametrize("c", _cases(), ids=_id)
def test_fused_equals_two_launches_and_the_restatement(c):
    run = _Run(c)
    for seed in _seeds(run.E, c["eps"], c["base"], c["step"]):
        got = run.fused(seed)
        greedy, two = run.two_launches(seed)
        _equal(got, two, "fused against act + select_actions")
        _equal(got, run.restated(seed, greedy), "fused against the restatement")
        _equal(got, run.fused(seed), "fused against a second launch")
        assert int(got[2].sum()) == {0.0: 0, 1.0: run.E}.get(c["eps"], int(got[2].sum()))


# ---- 2
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("EN", ((4, 64),) + AXES)
def test_an_exploring_colonys_inputs_do_not_matter(EN, fmt):
    import torch
    for eps in (0.5, 1.0):
        c = dict(BASE, EN=EN, fmt=fmt, eps=eps)
        run = _Run(c)
        seed = _seeds(run.E, eps, c["base"], c["step"])[0]
        ex = torch.from_numpy(A.explores(seed, c["step"], c["base"], run.E, eps))
        assert bool(ex.all()) if eps == 1.0 else (bool(ex.any()) and not bool(ex.all()))
        want = run.fused(seed)
        obs, ast = run.obs.clone(), run.ast.clone()
        obs[ex.cuda()] = float("nan")
        ast[ex.cuda()] = float("nan")
        assert int(torch.isnan(obs.float()).sum()) == int(ex.sum()) * run.N * c["F"]
        _equal(run.fused(seed, obs=obs, ast=ast), want, "NaN over the exploring colonies, epsilon %g" % eps)


# ---- 3
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("EN", AXES + ((5, 17),))
def test_q_out_is_written_for_the_other_colonies_only(EN, fmt):
    import torch
    c = dict(BASE, EN=EN, fmt=fmt)
    run = _Run(c)
    seed = _seeds(run.E, c["eps"], c["base"], c["step"])[0]
    q = torch.full((run.M, run.NQ), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
    want = torch.empty((run.M, run.NQ), dtype=torch.float32, device="cuda")
    got = run.fused(seed, logits=q)
    _, two = run.two_launches(seed, logits=want)
    _equal(got, two, "with q_out")
    ex = got[2].bool().repeat_interleave(run.N)
    assert 0 < int(ex.sum()) < run.M
    q, want = q.cpu(), want.cpu()
    assert same_bits(q[~ex], want[~ex])
    assert bool((q[ex].view(torch.int32) == PATTERN).all())


# ---- 4
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("EN,eps", (((7, 33), 0.5), ((5, 17), 0.5), ((1, 1), 0.5), ((1, 1), 1.0), ((3, 1), 0.5), ((7, 33), 1.0)))
def test_nothing_else_is_written(EN, eps, fmt):
    import torch
    c = dict(BASE, EN=EN, fmt=fmt, eps=eps)
    run = _Run(c)
    M, E, NQ, G = run.M, run.E, run.NQ, 64
    assert M % 8 != 0
    for seed in _seeds(E, eps, c["base"], c["step"]):
        want = run.fused(seed)
        bufs = {k: torch.full((G + n + G,), 0xA5, dtype=torch.uint8, device="cuda") for k, n in
                (("rot", M), ("ph", M), ("ex", E), ("q", 4 * NQ * M))}
        rot, ph = (bufs[k][G:G + M].view(torch.int8) for k in ("rot", "ph"))
        ex = bufs["ex"][G:G + E]
        q = bufs["q"][G:G + 4 * NQ * M].view(torch.float32).view(M, NQ)
        run.pol.act_select(run.obs, run.ast, seed=seed, step=c["step"], env_id_base=c["base"], n_envs=E, n_ants=run.N,
                           epsilon=eps, out=(rot, ph), explored=ex, logits=q)
        _equal((rot.cpu(), ph.cpu(), ex.cpu()), want, "carved out of larger buffers")
        for k, b in bufs.items():
            assert bool((b[:G] == 0xA5).all()) and bool((b[-G:] == 0xA5).all()), k
        before = {k: b.clone() for k, b in bufs.items()}
        run.pol.act_select(run.obs, run.ast, seed=seed, step=c["step"], env_id_base=c["base"], n_envs=E, n_ants=run.N,
                           epsilon=eps, out=(rot, ph), explored=None, logits=None)  # neither optional output
        assert all(torch.equal(bufs[k], before[k]) for k in bufs)


# ---- 5
def test_acting_against_the_reference(tmp_path):
    import torch
    from antsrl_amd.agent import ReworkAgent
    sd, rec = R.load_model("spread")
    path = str(tmp_path / "spread.h5")
    torch.save(sd, path)
    T = rec["obs"].shape[0]
    for fused in (True, False):
        ag = ReworkAgent(epsilon=0.0, seed=3, fused_select=fused)
        ag.setup(make_env(1, 64))
        ag.load_model(path)
        for training in (False, True):  # epsilon 0 explores nothing
            for t in range(T):
                obs = torch.from_numpy(rec["obs"][t]).reshape(1, 64, 7, 7, 6)
                rot, ph = ag.get_action(obs, torch.from_numpy(rec["agent_state"][t]).reshape(1, 64, 2), training)
                assert rot.shape == ph.shape == (1, 64) and rot.data_ptr() == ag._rot.data_ptr()
                assert torch.equal(rot.cpu().view(-1), torch.from_numpy(rec["rotation"][t]).view(-1).to(torch.int8)), (fused, training, t)
                assert torch.equal(ph.cpu().view(-1), torch.from_numpy(rec["pheromone"][t]).view(-1).to(torch.int8)), (fused, training, t)
        assert ag.step_counter == 2 * T and ag._action_step == 2 * T - 1


# ---- 6
def _agent(**kw):
    from antsrl_amd.agent import ReworkAgent
    return ReworkAgent(epsilon=0.5, learning_rate=1e-3, min_replay=500, replay_size=3000, seed=7, **kw)


def _check_loop(ag, losses, host_losses, acts, host_acts, tr, rm, synced_after_done, steps, E, N, ends):
    import torch
    assert len(rm) == min(3000, steps * E * N) and tr.step_count == steps - 1  # 256 rows after step 0: below min_replay
    assert len(synced_after_done) == ends and all(synced_after_done) and tr.syncs == ends  # synced after every done
    for t, (x, y) in enumerate(zip(losses, host_losses)):
        assert (x == 0 and y == 0) or float(x) == float(y), "loss, step %d" % t
    for t, (a, b) in enumerate(zip(acts, host_acts)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "actions, step %d" % t
    same_rings(ag.replay_memory, rm)
    assert ag.trainer.step_count == tr.step_count and ag.trainer.syncs == tr.syncs
    assert torch.equal(ag.trainer.model, tr.model) and torch.equal(ag.trainer.target, tr.target)
    assert torch.equal(ag.trainer._adam, tr._adam)
    assert same_bits(ag.policy.collapsed.cpu(), tr.policy.collapsed.cpu())


@pytest.mark.parametrize("fused", (True, False))
def test_the_loop_equals_the_loop_driven_entry_by_entry(fused):
    import torch
    from antsrl_amd.train import ReworkTrainer
    steps, E, N = 27, 4, 64
    ag = _agent(fused_select=fused)
    r = drive_loop(ag, ReworkTrainer, 264, True, lambda tr: torch.equal(tr.target, tr.model), steps, E, N, max_time=12)
    # (the harness's environments are reset once and never regenerate: their timestep passes max_time once, so drive_loop
    # crosses ONE episode end however long it runs; the loop below restarts its environments and crosses two)
    _check_loop(ag, r.losses, r.host_losses, r.acts, r.host_acts, r.trainer, r.ring, r.synced_after_done, steps, E, N, 1)
    assert torch.equal(r.env_a.obs, r.env_b.obs)
    assert ag.step_counter == steps


def _restart(env, episode, activation):
    """The next episode, as main.py:69-79 starts one: a new world, every pheromone activation x 10, the first observation."""
    from antsrl_amd.synth import synth_init
    env.reset(synth_init(env.cfg, seed=5 + episode, n_food_discs=6, food_rmin=3, food_rmax=6))
    env.set_activation(activation)
    return env.observe()


@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("fmt", FORMATS)
def test_the_loop_over_two_episodes_in_both_formats(fmt, fused):
    """drive_loop's comparison with what the harness does not build: bfloat16 environments, and a second episode (both
    environments are restarted when an episode ends, so the run crosses two episode ends and syncs the target twice).
    Every rollout_step runs under the sync debug mode; the same loop is then driven from the host, entry by entry."""
    import torch
    from agent_harness import ptr, stream
    from antsrl_amd import _lib
    from antsrl_amd import config as cm
    from antsrl_amd.replay import DeviceReplayMemory
    from antsrl_amd.train import ReworkTrainer
    lib = _lib.load()
    steps, E, N, max_time = 28, 4, 64, 12
    env_a, env_b = (make_env(E, N, max_time, dtype=getattr(torch, fmt)) for _ in range(2))
    activation = torch.full((E, N, 2), 10.0, device=env_a.device)
    ag = _agent(fused_select=fused)
    ag.setup(env_a)
    ag.initialize(env_a)
    env_a.observe()
    torch.cuda.synchronize()
    losses, acts, episode = [], [], 0
    for t in range(steps):
        done = env_a.query(cm.Q_TIMESTEP) == max_time
        torch.cuda.set_sync_debug_mode("error")  # the fused loop reads nothing back
        try:
            losses.append(ag.rollout_step(env_a))
        finally:
            torch.cuda.set_sync_debug_mode(0)
        acts.append((ag._rot.clone(), ag._ph.clone()))
        if done:
            episode += 1
            _restart(env_a, episode, activation)
    assert episode == 2
    tr = ReworkTrainer(294, env_b.device, lr=1e-3, seed=7)
    rm = DeviceReplayMemory(3000, (7, 7, 6), [2], [2], device=env_b.device)
    gen = torch.Generator(device=env_b.device)
    gen.manual_seed(7)
    env_b.set_activation(activation)
    obs, ast, _ = env_b.observe()
    assert obs.dtype == getattr(torch, fmt)
    host_losses, host_acts, synced, episode = [], [], [], 0
    for t in range(steps):
        rot, ph = (x.reshape(-1).clone() for x in tr.policy.act(obs, ast, env=env_b))
        _lib.check(lib.antsrl_agent_select_actions(7, t, 0, E, N, 0.5, 3, 3, ptr(rot), ptr(ph), None, stream()))
        host_acts.append((rot, ph))
        rm.record_pre(obs, ast, None, rot, ph, n_envs=E, n_ants=N, seed=7, step=t)
        done = env_b.query(cm.Q_TIMESTEP) == max_time
        env_b.step_update(rot.view(E, N), ph.view(E, N))
        rm.record_post(env_b.obs, env_b.agent_state, None, env_b.reward.view(-1), env_b.done)
        host_losses.append(tr.train(rm, done, minibatch=264, min_replay=500, generator=gen))
        if done:
            synced.append(torch.equal(tr.target, tr.model))
            episode += 1
            obs, ast, _ = _restart(env_b, episode, activation)
    _check_loop(ag, losses, host_losses, acts, host_acts, tr, rm, synced, steps, E, N, 2)
    assert torch.equal(env_a.obs, env_b.obs)


# ---- 7
def test_save_and_load(tmp_path):
    import torch
    from antsrl_amd.agent import ReworkAgent
    from antsrl_amd.policy import REWORK_LAYERS, rework_param_shapes
    env = make_env()
    a, b = ReworkAgent(seed=1, rotations=5, pheromones=2), ReworkAgent(seed=2, rotations=5, pheromones=2)
    a.setup(env)
    b.setup(env)
    path = str(tmp_path / "rework.h5")
    a.save_model(path)
    sd = torch.load(path)
    assert list(sd) == [l + s for l in REWORK_LAYERS for s in (".weight", ".bias")] and len(sd) == 20
    for l, (o, i) in rework_param_shapes(294, 5, 2).items():
        assert tuple(sd[l + ".weight"].shape) == (o, i) and tuple(sd[l + ".bias"].shape) == (o,)
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd.values())
    assert not torch.equal(b.trainer.model, a.trainer.model)
    version = b.trainer.version
    b.load_model(path)
    assert b.trainer.version == version + 1
    assert torch.equal(b.trainer.model, a.trainer.model) and torch.equal(b.trainer.target, b.trainer.model)
    assert same_bits(b.policy.collapsed.cpu(), a.policy.collapsed.cpu())
    env.observe()
    ra, pa = (t.clone() for t in a.get_action(env.obs, env.agent_state, False, env=env))
    rb, pb = b.get_action(env.obs, env.agent_state, False, env=env)
    assert torch.equal(ra, rb) and torch.equal(pa, pb) and ra.shape == (4, 64)
    c = ReworkAgent(seed=3, rotations=5, pheromones=2)
    c.setup(env, trained_model=path)  # setup's own load
    assert torch.equal(c.trainer.model, a.trainer.model) and torch.equal(c.trainer.target, a.trainer.model)


# ---- 8
def test_the_loss_falls_on_one_minibatch():
    import torch
    from antsrl_amd.agent import ReworkAgent
    from test_rework_train_fixture import FIXTURE, fixture_arrays
    arrays, idx = fixture_arrays(np.load(FIXTURE))
    arrays, idx = tuple(a.cuda().contiguous() for a in arrays), idx[0].cuda()
    ag = ReworkAgent(learning_rate=1e-3, seed=1)
    ag.setup(make_env(1, 64))
    tr = ag.trainer
    t0 = tr.target.clone()
    losses = [tr.step(arrays, idx, keep_grads=False).clone() for _ in range(200)]  # no sync: the target stays frozen
    first, last = float(losses[0]), float(losses[-1])
    print("\nMEASURED loss on one minibatch of the fixture's rows, 200 steps at lr 1e-3: %.5f -> %.5f" % (first, last))
    assert torch.equal(tr.target, t0) and last < first
