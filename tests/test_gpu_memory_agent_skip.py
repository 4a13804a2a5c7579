"""Skipping the net for exploring environments (antsrl_agent_plan, antsrl_policy_memory_tiles, MemoryPolicy.act(tiles=),
MemoryAgent(skip_explored=True)) against the plan's numpy restatement (tests/memory_agent_plan_ref.py), the full forward
(antsrl_policy_memory_ex) and the loop without the switch.  An ant's outputs depend only on its own inputs and the draws are
counter-based, so every comparison here is bit for bit.  The out-of-range list entries of the forward test are refused by
a compare in the kernel, before they could become an address."""
import ctypes as C

import numpy as np
import pytest

import memory_agent_plan_ref as P
from agent_harness import make_env as _env
from agent_harness import ptr as _p
from agent_harness import same_rings as _same_rings
from agent_harness import stream as _stream

pytestmark = pytest.mark.gpu


def _plan(seed, step, base, E, N, eps):
    """(tiles int32 [T] pre-filled with -7, n_live int32 [1]) after antsrl_agent_plan."""
    import torch
    from antsrl_amd import _lib
    tiles = torch.full((P.n_tiles(E, N),), -7, dtype=torch.int32, device="cuda")
    n_live = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().antsrl_agent_plan(seed, step, base, E, N, eps, _p(tiles), _p(n_live), _stream()), "agent_plan")
    return tiles, n_live


# test_select_equals_the_restatement's sweep (without its mem column), plus N in {50, 512} and epsilon in {0, 1}
@pytest.mark.parametrize("E,N,eps,step,base", [(4, 64, 0.5, 0, 0), (7, 33, 0.3, 5, 0), (16, 512, 0.5, 123456789, 0),
                                               (5, 17, 0.5, 2, 3), (8, 64, 0.0, 1, 0), (8, 64, 1.0, 1, 0),
                                               (3, 1, 0.5, 9, 1 << 20), (64, 64, 0.1, 4, 0),
                                               (6, 50, 0.5, 3, 0), (9, 50, 0.9, 1, 7), (6, 50, 0.0, 3, 0), (6, 50, 1.0, 3, 0),
                                               (40, 512, 0.9, 7, 0), (40, 512, 0.1, 8, 2), (4, 512, 0.0, 0, 0), (4, 512, 1.0, 0, 0),
                                               (1024, 512, 0.5, 11, 0)])
def test_plan_equals_the_restatement(E, N, eps, step, base):
    rng = np.random.default_rng(E * 1000 + N)
    seed = int(rng.integers(0, 1 << 62)) * 3 + 1
    tiles, n_live = _plan(seed, step, base, E, N, eps)
    want = P.live_tiles(seed, step, base, E, N, eps)
    n = int(n_live.item())
    print("plan E=%d N=%d eps=%g: n_live %d of %d (restatement %d)" % (E, N, eps, n, P.n_tiles(E, N), want.size))
    assert n == want.size
    assert np.array_equal(tiles[:n].cpu().numpy(), want)
    if eps == 0.0:
        assert n == P.n_tiles(E, N)
    if eps == 1.0:
        assert n == 0


# ---- the tile-list forward against the full forward
def _forward(pol, obs, ast, mem_in, mem_out, rot, ph, q, lst=None):
    """antsrl_policy_memory_ex, or antsrl_policy_memory_tiles with lst = (tiles, n_live), on the caller's buffers."""
    from antsrl_amd import _lib
    lib, M = _lib.load(), mem_in.shape[0]
    fmt = 1 if obs.element_size() == 2 else 0
    head = (C.byref(pol.shape), pol._precision_id(), _p(pol.packed), _p(obs), fmt, _p(ast), _p(mem_in), M, _p(mem_out), _p(rot),
            _p(ph), _p(q))
    if lst is None:
        _lib.check(lib.antsrl_policy_memory_ex(*head, _stream()), "policy_memory_ex")
    else:
        _lib.check(lib.antsrl_policy_memory_tiles(*head, _p(lst[0]), _p(lst[1]), _stream()), "policy_memory_tiles")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("bf16_obs", [False, True])
@pytest.mark.parametrize("power,mem,E,N", [(4, 10, 4, 50), (5, 20, 9, 37)])  # M = 200, 333: no multiple of 32 or of 128
def test_tile_list_forward_equals_the_full_forward(precision, bf16_obs, power, mem, E, N):
    import torch
    from antsrl_amd.policy import MemoryPolicy
    M, F = E * N, 294
    T = P.n_tiles(E, N)
    g = torch.Generator(device="cuda").manual_seed(1000 * power + M + bf16_obs)
    pol = MemoryPolicy(F, "cuda", power=power, mem_size=mem, seed=3, precision=precision)
    obs = (torch.rand((M, 7, 7, 6), device="cuda", generator=g) * 2 - 0.5).to(torch.bfloat16 if bf16_obs else torch.float32)
    ast = torch.rand((M, 2), device="cuda", generator=g)
    old = torch.rand((M, mem), device="cuda", generator=g) * 2 - 1
    # the full forward: the yardstick
    w_mem, w_q = torch.empty((M, mem), device="cuda"), torch.empty((M, 6), device="cuda")
    w_rot, w_ph = (torch.empty((M,), dtype=torch.int8, device="cuda") for _ in range(2))
    _forward(pol, obs, ast, old, w_mem, w_rot, w_ph, w_q)

    def dev(a):
        return torch.tensor(list(a), dtype=torch.int32, device="cuda")

    third = list(range(0, T, 3))
    spoiled = []
    for i, t in enumerate(third):  # the same list with entries outside [0, T) mixed in
        spoiled += [t] + ([-1] if i % 2 == 0 else [T + 5])
    spoiled = spoiled[:T]
    kept_of_spoiled = [t for t in spoiled if 0 <= t < T]
    planned, planned_n = _plan(77, 3, 0, E, N, 0.5)
    want_plan = P.live_tiles(77, 3, 0, E, N, 0.5)
    assert 0 < want_plan.size < T  # the case is a real subset
    lists = {
        "all": (dev(range(T)), dev([T]), range(T)),
        "all, n_live beyond T (clamped)": (dev(range(T)), dev([T + 100]), range(T)),
        "none": (dev(range(T)), dev([0]), []),
        "negative n_live": (dev(range(T)), dev([-3]), []),
        "every third": (dev(third + [0] * (T - len(third))), dev([len(third)]), third),
        "the plan's": (planned, planned_n, want_plan.tolist()),
        "descending": (dev(reversed(range(T))), dev([T]), range(T)),
        "with -1 and T + 5": (dev(spoiled + [0] * (T - len(spoiled))), dev([len(spoiled)]), kept_of_spoiled),
    }
    results = {}
    for name, (tl, nl, listed) in lists.items():
        ant_listed = torch.zeros((T * 32,), dtype=torch.bool, device="cuda")
        if len(listed):
            ant_listed.view(T, 32)[torch.tensor(list(listed), device="cuda")] = True
        ant_listed = ant_listed[:M]
        for in_place in (False, True):
            s_mem = old.clone() if in_place else torch.full((M, mem), -123.5, device="cuda")
            s_q = torch.full((M, 6), -123.5, device="cuda")
            s_rot, s_ph = (torch.full((M,), 99, dtype=torch.int8, device="cuda") for _ in range(2))
            mem_in = s_mem if in_place else old
            _forward(pol, obs, ast, mem_in, s_mem, s_rot, s_ph, s_q, (tl, nl))
            sentinel_mem = old if in_place else torch.full_like(old, -123.5)
            case = (name, in_place)
            assert torch.equal(s_rot, torch.where(ant_listed, w_rot, torch.full_like(w_rot, 99))), case
            assert torch.equal(s_ph, torch.where(ant_listed, w_ph, torch.full_like(w_ph, 99))), case
            assert torch.equal(s_mem, torch.where(ant_listed[:, None], w_mem, sentinel_mem)), case
            assert torch.equal(s_q, torch.where(ant_listed[:, None], w_q, torch.full_like(w_q, -123.5))), case
            results[case] = (s_rot, s_ph, s_mem, s_q)
    # the out-of-range entries are skipped: the same outputs as the list without them
    for in_place in (False, True):
        for x, y in zip(results[("with -1 and T + 5", in_place)], results[("every third", in_place)]):
            assert torch.equal(x, y)
    # MemoryPolicy.act(tiles=): the same entry behind the public surface; None is today's path
    r0, p0, m0 = pol.act(obs, ast, memory=old, out=torch.empty_like(old))
    assert torch.equal(r0, w_rot) and torch.equal(p0, w_ph) and torch.equal(m0, w_mem)
    pol._rot.fill_(99)
    pol._ph.fill_(99)
    out = torch.full_like(old, -123.5)
    r1, p1, m1 = pol.act(obs, ast, memory=old, out=out, tiles=(lists["every third"][0], lists["every third"][1]))
    for got, want in zip((r1, p1, m1), results[("every third", False)][:3]):
        assert torch.equal(got, want)


# ---- the loop
def _agent(eps, state_memory="reference", **kw):
    from antsrl_amd.agent import MemoryAgent
    return MemoryAgent(epsilon=eps, discount=0.99, learning_rate=1e-3, min_replay=500, replay_size=3000, seed=7,
                       state_memory=state_memory, **kw)


def _same_end_state(a, b):
    import torch
    _same_rings(a.replay_memory, b.replay_memory)
    # masters of every parameter, Adam's moments and the packs live in these two state buffers
    assert torch.equal(a.trainer._model, b.trainer._model) and torch.equal(a.trainer._target, b.trainer._target)
    assert (a.trainer.step_count, a.trainer.syncs) == (b.trainer.step_count, b.trainer.syncs)
    sa, sb = a.trainer.state_dict(), b.trainer.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(torch.equal(v, b.policy.params[k]) for k, v in a.policy.params.items())
    assert torch.equal(a.previous_memory, b.previous_memory)


@pytest.mark.parametrize("state_memory", ["reference", "carried"])
@pytest.mark.parametrize("eps", [0.1, 0.9])
@pytest.mark.parametrize("K,bf16_obs,precision", [(None, False, "bf16"), (32, True, "bf16"), (None, False, "fp32")])
def test_the_loop_with_skip_explored_equals_the_loop_without(state_memory, eps, K, bf16_obs, precision):
    import torch
    steps, E, N, max_time = 36, 4, 64, 12
    dt = torch.bfloat16 if bf16_obs else torch.float32
    envs = [_env(E, N, max_time, dtype=dt) for _ in range(2)]
    ags = [_agent(eps, state_memory, record_per_step=K, precision=precision, skip_explored=s) for s in (False, True)]
    for ag, env in zip(ags, envs):
        ag.setup(env)
        ag.initialize(env)
        env.observe()
    off, on = ags
    losses, explored_steps, skipped = ([], []), 0, 0
    for t in range(steps):
        for i, (ag, env) in enumerate(zip(ags, envs)):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")  # plan, tile-list forward, select: nothing is read back
            try:
                losses[i].append(ag.rollout_step(env))
            finally:
                torch.cuda.set_sync_debug_mode(0)
        assert torch.equal(off.policy._rot, on.policy._rot) and torch.equal(off.policy._ph, on.policy._ph), t  # the actions
        assert torch.equal(off.previous_memory, on.previous_memory), t                                          # carried memory
        assert torch.equal(off._explored, on._explored), t
        assert torch.equal(envs[0].obs, envs[1].obs) and torch.equal(envs[0].reward, envs[1].reward), t
        explored_steps += int(on._explored.sum().item())
        skipped += on._tiles.numel() - int(on._n_live.item())
    assert 0 < explored_steps < steps * E and skipped == explored_steps * (N // 32)  # the switch did skip tiles
    for x, y in zip(*losses):
        assert (torch.is_tensor(x) and torch.equal(x, y)) if torch.is_tensor(y) else x == y == 0
    assert off.trainer.step_count >= 18
    _same_end_state(off, on)


def test_the_reference_surface_by_hand_with_skip_explored_equals_rollout_step():
    import torch
    from antsrl_amd import config as cm
    steps, max_time = 14, 6
    env_a, env_b = _env(max_time=max_time), _env(max_time=max_time)
    a, b = _agent(0.5, skip_explored=True), _agent(0.5, skip_explored=True)
    for ag, env in ((a, env_a), (b, env_b)):
        ag.setup(env)
        ag.initialize(env)
    env_a.observe()
    a.run(env_a, steps)
    obs, ast, _ = env_b.observe()
    for s in range(steps):  # main.py:92-131
        obs, ast = obs.clone(), ast.clone()  # the environment writes every observation into the same buffer
        action = b.get_action(obs, ast, True)
        done_host = env_b.query(cm.Q_TIMESTEP) == max_time
        new_obs, new_ast, reward, done = env_b.step(*action[:2])
        b.update_replay_memory(obs, ast, action, reward, new_obs, new_ast, done)
        b.train(done_host, s)
        obs, ast = new_obs, new_ast
        env_b.update()
    assert b.trainer.step_count > 0 and b.trainer.syncs == 1
    _same_end_state(a, b)


def test_nothing_changes_when_the_switch_is_off_or_the_agent_is_not_training():
    import torch
    from antsrl_amd.agent import MemoryAgent
    assert MemoryAgent().skip_explored is False
    envs = [_env() for _ in range(3)]
    ags = [_agent(0.5), _agent(0.5, skip_explored=True), _agent(0.5, skip_explored=False)]
    for ag, env in zip(ags, envs):
        ag.setup(env)
        ag.initialize(env)
        env.observe()
        ag._tiles.fill_(-7)
        ag._n_live.fill_(-7)
    plain, not_training, off = ags
    for t in range(6):
        want = plain.rollout_step(envs[0], training=False)
        assert want == 0 and not_training.rollout_step(envs[1], training=False) == 0
        for x, y in ((plain.policy._rot, not_training.policy._rot), (plain.policy._ph, not_training.policy._ph),
                     (plain.previous_memory, not_training.previous_memory), (envs[0].obs, envs[1].obs)):
            assert torch.equal(x, y), t
        off.rollout_step(envs[2])
    # no plan ran in either: training=False takes the full forward, and so does skip_explored=False while training
    for ag in (not_training, off):
        assert int(ag._n_live.item()) == -7 and bool((ag._tiles == -7).all())
    assert len(off.replay_memory) == 6 * 256 and off.trainer.step_count > 0
