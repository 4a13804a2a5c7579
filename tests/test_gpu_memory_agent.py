"""The memory agent on the device (antsrl_agent_select, antsrl_replay_record_pre / _post, DeviceReplayMemory.record_*,
MemoryAgent) against the numpy restatement of tests/memory_agent_ref.py, the reference's own recorded run, and the same
loop assembled from the parts that existed before (MemoryPolicy.act, cloned observations + DeviceReplayMemory.extend,
MemoryTrainer.train).  Everything here is copying or integer work: every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import memory_agent_ref as R
from agent_harness import make_env as _env
from agent_harness import ptr as _p
from agent_harness import same_rings as _same_rings

pytestmark = pytest.mark.gpu

CONTRACT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract")


def _select(seed, step, base, E, N, eps, rot, ph, old, new, explored=None, n_rot=3, n_ph=3):
    import torch
    from antsrl_amd import _lib
    _lib.check(_lib.load().antsrl_agent_select(seed, step, base, E, N, eps, n_rot, n_ph, old.shape[-1], _p(rot), _p(ph), _p(old),
                                               _p(new), _p(explored), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "agent_select")


@pytest.mark.parametrize("E,N,mem,eps,step,base", [(4, 64, 20, 0.5, 0, 0), (7, 33, 20, 0.3, 5, 0), (16, 512, 20, 0.5, 123456789, 0),
                                                   (5, 17, 7, 0.5, 2, 3), (8, 64, 20, 0.0, 1, 0), (8, 64, 20, 1.0, 1, 0),
                                                   (3, 1, 1, 0.5, 9, 1 << 20), (64, 64, 32, 0.1, 4, 0)])
def test_select_equals_the_restatement(E, N, mem, eps, step, base):
    import torch
    rng = np.random.default_rng(E * 1000 + N)
    seed = int(rng.integers(0, 1 << 62)) * 3 + 1
    rot, ph = rng.integers(-1, 2, (E, N)).astype(np.int8), rng.integers(0, 3, (E, N)).astype(np.int8)
    old, new = rng.random((E, N, mem), np.float32), rng.random((E, N, mem), np.float32)
    d = [torch.from_numpy(a.copy()).cuda() for a in (rot, ph, old, new)]
    expl = torch.full((E,), 7, dtype=torch.uint8, device="cuda")
    _select(seed, step, base, E, N, eps, *d, explored=expl)
    w_rot, w_ph, w_new, w_ex = R.select(seed, step, base, eps, 3, 3, rot, ph, old, new)
    assert np.array_equal(d[0].cpu().numpy(), w_rot) and np.array_equal(d[1].cpu().numpy(), w_ph)
    assert np.array_equal(d[3].cpu().numpy(), w_new) and np.array_equal(d[2].cpu().numpy(), old)
    assert np.array_equal(expl.cpu().numpy().astype(bool), w_ex)
    if eps == 0.0:
        assert not w_ex.any() and np.array_equal(d[3].cpu().numpy(), new) and np.array_equal(d[0].cpu().numpy(), rot)
    if eps == 1.0:
        assert w_ex.all() and np.array_equal(d[3].cpu().numpy(), old)
    # in place over one buffer (mem_old == mem_next): the actions alike, the memory untouched
    d2 = [torch.from_numpy(a.copy()).cuda() for a in (rot, ph, old)]
    _select(seed, step, base, E, N, eps, d2[0], d2[1], d2[2], d2[2])
    assert np.array_equal(d2[0].cpu().numpy(), w_rot) and np.array_equal(d2[2].cpu().numpy(), old)


def test_select_shards_equal_the_full_batch():
    import torch
    E, N, mem = 8, 48, 20
    rng = np.random.default_rng(1)
    rot, ph = rng.integers(-1, 2, (E, N)).astype(np.int8), rng.integers(0, 3, (E, N)).astype(np.int8)
    old, new = rng.random((E, N, mem), np.float32), rng.random((E, N, mem), np.float32)
    full = [torch.from_numpy(a.copy()).cuda() for a in (rot, ph, old, new)]
    _select(77, 4, 0, E, N, 0.5, *full)
    for base in (0, E // 2):
        sl = slice(base, base + E // 2)
        part = [torch.from_numpy(a[sl].copy()).cuda() for a in (rot, ph, old, new)]
        _select(77, 4, base, E // 2, N, 0.5, *part)
        for f, q in zip(full, part):
            assert torch.equal(f[sl], q)


def test_recording_the_references_own_run():
    import torch
    from antsrl_amd.replay import DeviceReplayMemory
    z = np.load(os.path.join(CONTRACT, "agent_contract.npz"))
    n = z["rot"].shape[1]
    rm = DeviceReplayMemory(50000, (7, 7, 6), [22], [2])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)  # noqa: E731
    obs, ast = dev(z["obs0"], torch.float32), dev(z["agent_state0"], torch.float32)
    mem = torch.zeros((n, 20), device="cuda")
    for s in range(10):
        rm.record_pre(obs, ast, mem, dev(z["rot"][s], torch.int8), dev(z["ph"][s], torch.int8), n_envs=1, n_ants=n, step=s)
        obs, ast = dev(z["obs"][s], torch.float32), dev(z["agent_state"][s], torch.float32)
        rm.record_post(obs, ast, mem, dev(z["reward"][s], torch.float32), bool(z["done"][s]))
    assert len(rm) == 160 and rm.head == 160
    assert np.array_equal(rm.states[:160].cpu().numpy(), z["replay_states"])
    assert np.array_equal(rm.actions[:160].cpu().numpy(), z["replay_actions"])
    assert np.array_equal(rm.rewards[:160].cpu().numpy(), z["replay_rewards"])
    assert np.array_equal(rm.dones[:160].cpu().numpy(), np.repeat(z["done"], n))


@pytest.mark.parametrize("P,bf16,pitch", [((7, 7, 6), False, 0), ((7, 7, 7), False, 0), ((7, 7, 6), True, 0),
                                          ((7, 7, 7), True, 0), ((7, 7, 6), False, 320), ((7, 7, 7), False, 352),
                                          ((7, 7, 7), True, 384), ((3, 3, 1), False, 0), ((1, 1, 2), True, 0)])
def test_record_equals_extend(P, bf16, pitch):
    """Seeded random steps through record_pre / record_post and through extend on the same rows: a ring that wraps inside
    a call, K > max_len, K < M (rows picked by the restatement's indices), per-environment done."""
    import torch
    from antsrl_amd.replay import DeviceReplayMemory
    E, N, mem, L = 3, 50, 20, 400
    M, F = E * N, int(np.prod(P))
    g = torch.Generator(device="cuda").manual_seed(F + pitch + bf16)
    a, b = DeviceReplayMemory(L, P, [2 + mem], [2]), DeviceReplayMemory(L, P, [2 + mem], [2])
    a.head = b.head = 3  # odd rows first: both alignments of a 1 176-byte ring row come up
    dt = torch.bfloat16 if bf16 else torch.float32

    def observation():
        buf = torch.rand((M, pitch or F), device="cuda", generator=g).to(dt)
        return buf, buf[:, :F]

    for step, K in enumerate([M, 40, M, 7, 1, 149, M, 64]):  # 400-row ring: the 6th call wraps
        buf0, obs0 = observation()
        buf1, obs1 = observation()
        ast0, ast1 = (torch.rand((M, 2), device="cuda", generator=g) for _ in range(2))
        m0, m1 = (torch.rand((M, mem), device="cuda", generator=g) for _ in range(2))
        rot = torch.randint(-1, 2, (M,), device="cuda", generator=g).to(torch.int8)
        ph = torch.randint(0, 3, (M,), device="cuda", generator=g).to(torch.int8)
        rew = torch.randn((M,), device="cuda", generator=g)
        done = (torch.rand((E,), device="cuda", generator=g) < 0.4).to(torch.uint8)
        a.record_pre(buf0, ast0, m0, rot, ph, n_envs=E, n_ants=N, k=K, seed=99, step=step, env_id_base=2, obs_pitch=pitch)
        a.record_post(buf1, ast1, m1, rew, done)
        idx = torch.from_numpy(R.sample_indices(99, step, 2, M, K)).cuda()
        b.extend(obs0.float()[idx], torch.cat([ast0, m0], 1)[idx], (rot.long()[idx] + 1, ph.long()[idx]), rew[idx],
                 obs1.float()[idx], torch.cat([ast1, m1], 1)[idx], done.repeat_interleave(N)[idx])
        _same_rings(a, b)
    # K > max_len: only the newest max_len entries
    c, d = DeviceReplayMemory(100, P, [2 + mem], [2]), DeviceReplayMemory(100, P, [2 + mem], [2])
    c.head = d.head = 97
    c.record_pre(buf0, ast0, m0, rot, None, n_envs=E, n_ants=N, obs_pitch=pitch)  # pheromone None: 1, as extend
    c.record_post(buf1, ast1, m1, rew, done.bool())
    d.extend(obs0.float(), torch.cat([ast0, m0], 1), (rot.long() + 1, None), rew, obs1.float(), torch.cat([ast1, m1], 1), done)
    _same_rings(c, d)


def _agent(state_memory="reference", **kw):
    from antsrl_amd.agent import MemoryAgent
    return MemoryAgent(epsilon=0.5, discount=0.99, learning_rate=1e-3, min_replay=500, replay_size=3000, seed=7,
                       state_memory=state_memory, **kw)


def _same_agents_state(ag, tr, replay, memory):
    import torch
    assert torch.equal(ag.trainer._model, tr._model) and torch.equal(ag.trainer._target, tr._target)  # masters, Adam, packs
    assert ag.trainer.step_count == tr.step_count and ag.trainer.syncs == tr.syncs
    assert all(torch.equal(v, tr.policy.params[k]) for k, v in ag.policy.params.items())  # the acting (target) net
    _same_rings(ag.replay_memory, replay)
    assert torch.equal(ag.previous_memory, memory)


@pytest.mark.parametrize("state_memory", ["reference", "carried"])
def test_the_loop_equals_the_loop_assembled_from_the_old_parts(state_memory):
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.replay import DeviceReplayMemory
    from antsrl_amd.train import MemoryTrainer
    steps, E, N, max_time = 36, 4, 64, 12
    env_a, env_b = _env(E, N, max_time), _env(E, N, max_time)
    ag = _agent(state_memory)
    ag.setup(env_a)
    ag.initialize(env_a)
    env_a.observe()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # the fused loop reads nothing back
    try:
        losses = ag.run(env_a, steps)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    # ---- the same loop from the parts that existed before
    M, F = E * N, 294
    tr = MemoryTrainer(F, env_b.device, discount=0.99, lr=1e-3, seed=7)
    replay = DeviceReplayMemory(3000, (7, 7, 6), [22], [2], device=env_b.device)
    gen = torch.Generator(device=env_b.device)
    gen.manual_seed(7)
    env_b.set_activation(torch.full((E, N, 2), 10.0, device=env_b.device))
    obs, ast, _ = env_b.observe()
    mem, nxt = torch.zeros((M, 20), device=env_b.device), torch.zeros((M, 20), device=env_b.device)
    want_losses, trained = [], 0
    for t in range(steps):
        rot, ph, _ = tr.policy.act(obs, ast, memory=mem, out=nxt)
        s = R.select(7, t, 0, 0.5, 3, 3, rot.cpu().numpy(), ph.cpu().numpy(), mem.view(E, N, 20).cpu().numpy(),
                     nxt.view(E, N, 20).cpu().numpy())
        rot, ph = torch.from_numpy(s[0]).to(env_b.device), torch.from_numpy(s[1]).to(env_b.device)
        nxt.copy_(torch.from_numpy(s[2]).view(M, 20))
        before = nxt if state_memory == "reference" else mem
        o, a = obs.reshape(M, 7, 7, 6).clone(), torch.cat([ast.reshape(M, 2), before], dim=1)
        done_host = env_b.query(cm.Q_TIMESTEP) == max_time
        new_obs, new_ast, rew, done = env_b.step_update(rot, ph)
        replay.extend(o, a, (rot.reshape(-1).long() + 1, ph.reshape(-1).long()), rew.reshape(-1), new_obs.reshape(M, 7, 7, 6),
                      torch.cat([new_ast.reshape(M, 2), nxt], dim=1), done)
        want_losses.append(tr.train(replay, done_host, minibatch=264, min_replay=500, generator=gen))
        trained += len(replay) >= 500
        mem, nxt = nxt, mem
        obs, ast = new_obs, new_ast
    assert trained >= 30 and tr.syncs == 1  # training started, and the episode's end synced the target
    for got, want in zip(losses, want_losses):
        assert (torch.is_tensor(got) and torch.equal(got, want)) if torch.is_tensor(want) else got == want == 0
    _same_agents_state(ag, tr, replay, mem)
    for x, y in ((env_a.obs, env_b.obs), (env_a.agent_state, env_b.agent_state), (env_a.reward, env_b.reward)):
        assert torch.equal(x, y)


def test_a_sampled_bfloat16_loop_runs_and_records_what_the_restatement_picks():
    import torch
    E, N, K = 4, 64, 32
    env = _env(E, N, dtype=torch.bfloat16)
    ag = _agent(record_per_step=K)
    ag.setup(env)
    ag.initialize(env)
    env.observe()
    first = env.obs.reshape(E * N, -1).float().clone()
    ag.run(env, 20)
    rm = ag.replay_memory
    assert len(rm) == 20 * K and rm.head == 20 * K
    assert torch.equal(rm.states[:K].reshape(K, -1), first[torch.from_numpy(R.sample_indices(7, 0, 0, E * N, K)).cuda()])
    assert ag.trainer.step_count == sum(1 for t in range(20) if (t + 1) * K >= 500)


def test_the_reference_surface_by_hand_equals_rollout_step(tmp_path):
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.agent import MemoryAgent
    steps, max_time = 14, 6
    env_a, env_b = _env(max_time=max_time), _env(max_time=max_time)
    a, b = _agent(), _agent()
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
    _same_agents_state(a, b.trainer, b.replay_memory, b.previous_memory)
    # save_model / load_model: the reference's 26 names in its order, and model, target and acting policy restored
    path = str(tmp_path / "model.h5")
    a.save_model(path)
    sd = torch.load(path)
    keys = [str(k) for k in np.load(os.path.join(CONTRACT, "memory_train_ref.npz"))["state_dict_keys"]]
    assert list(sd.keys()) == keys and len(keys) == 26
    c = MemoryAgent(seed=123)
    c.setup(env_b)
    assert not torch.equal(c.trainer.state_dict()["layer1.weight"], a.trainer.state_dict()["layer1.weight"])
    c.load_model(path)
    want = a.trainer.state_dict()
    for k in keys:
        assert torch.equal(c.trainer.state_dict()[k], want[k]) and torch.equal(c.trainer.target_state_dict()[k], want[k])
        assert torch.equal(c.policy.params[k], want[k])
    c.epsilon = 0.25  # settable, as main.py:149 anneals it
    assert c.epsilon == 0.25
