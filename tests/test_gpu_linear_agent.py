"""The linear agent on the device: the memory-less select and record entries against the memory agent's,
LinearTrainer against the device-contract restatement and the reference's recorded run (tests/linear_train_ref.py,
golden/contract/linear_train_ref.npz), CollectAgent's acting against the recorded actions, and its fused loop against the
same loop driven entry by entry, standalone and in-loop."""
import os

import numpy as np
import pytest

import linear_train_ref as L
import memory_agent_ref as R
from agent_harness import drive_loop, inloop_runs, linear_snapshot, twin_report
from agent_harness import random_linear_replay as _random_replay
from agent_harness import make_env as _env
from agent_harness import ptr as _p
from agent_harness import same_rings as _same_rings
from agent_harness import stream as _stream
from dqn_ref import RING

pytestmark = pytest.mark.gpu

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "linear_train_ref.npz")

# Bounds of test_step_equals_the_contract: about 4 x the worst figure the sweep prints (-s) on an MI355X, per batch size
# (DESIGN §7.11 and profiles/linear_agent_c5.json list the measured values).  What they cover is the order of fp32 sums: the
# restatement sums in float64 and rounds once, the device sums in fp32 (every product of bfloat16 operands is exact).
#                          measured worst: B <= 4096    B = 65 536
BOUND_GRAD = {False: 8e-7, True: 2.8e-6}    # 1.99e-7        6.89e-7     max |g - g_ref| / max |g_ref| per tensor
BOUND_LOSS = {False: 5e-7, True: 2e-6}      # 1.21e-7        5.01e-7     |loss - loss_ref| / loss_ref
BOUND_HEADS = 1e-4   # |p - p_ref| in units of one step of lr, from equal gradients: test_gpu_memory_train.py's bound
#                      (measured worst 3.73e-5: one ulp of a head weight near 0.1 against a step of 1e-4)


# ---- 1. select
@pytest.mark.parametrize("E,N,eps,step,base", [(4, 64, 0.0, 1, 0), (8, 64, 0.1, 3, 0), (7, 33, 0.5, 5, 0), (5, 17, 0.5, 2, 3),
                                               (8, 64, 1.0, 1, 0), (3, 1, 0.5, 9, 1 << 20), (16, 512, 0.1, 123456789, 7)])
def test_select_actions_equals_select_and_the_restatement(E, N, eps, step, base):
    import torch
    from antsrl_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(E * 1000 + N)
    seed = int(rng.integers(0, 1 << 62)) * 3 + 1
    rot, ph = rng.integers(-1, 2, (E, N)).astype(np.int8), rng.integers(0, 3, (E, N)).astype(np.int8)
    mem = rng.random((E, N, 4), np.float32)
    a = [torch.from_numpy(x.copy()).cuda() for x in (rot, ph)]
    b = [torch.from_numpy(x.copy()).cuda() for x in (rot, ph, mem, mem)]
    ea, eb = (torch.full((E,), 7, dtype=torch.uint8, device="cuda") for _ in range(2))
    _lib.check(lib.antsrl_agent_select_actions(seed, step, base, E, N, eps, 3, 3, _p(a[0]), _p(a[1]), _p(ea), _stream()))
    _lib.check(lib.antsrl_agent_select(seed, step, base, E, N, eps, 3, 3, 4, _p(b[0]), _p(b[1]), _p(b[2]), _p(b[3]), _p(eb),
                                       _stream()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(ea, eb)
    w_rot, w_ph, _, w_ex = R.select(seed, step, base, eps, 3, 3, rot, ph, mem, mem.copy())
    assert np.array_equal(a[0].cpu().numpy(), w_rot) and np.array_equal(a[1].cpu().numpy(), w_ph)
    assert np.array_equal(ea.cpu().numpy().astype(bool), w_ex)
    _lib.check(lib.antsrl_agent_select_actions(seed, step, base, E, N, eps, 3, 3, _p(a[0]), _p(a[1]), None, _stream()))  # explored NULL


# ---- 2. record
@pytest.mark.parametrize("P,bf16,pitch", [((7, 7, 6), False, 0), ((7, 7, 6), True, 0), ((7, 7, 7), False, 352),
                                          ((7, 7, 7), True, 384), ((3, 3, 1), False, 0)])
def test_record_plain_equals_record(P, bf16, pitch):
    """The same seeded steps through the memory-less halves and through the halves with a memory: every shared array bit
    for bit, agent_states the 2-float rows.  K = M and K < M, a ring that wraps inside a call, K > max_len."""
    import torch
    from antsrl_amd.replay import DeviceReplayMemory
    E, N, mem, Lr = 3, 50, 20, 400
    M, F = E * N, int(np.prod(P))
    g = torch.Generator(device="cuda").manual_seed(F + pitch + bf16)
    a, b = DeviceReplayMemory(Lr, P, [2], [2]), DeviceReplayMemory(Lr, P, [2 + mem], [2])
    a.head = b.head = 3
    dt = torch.bfloat16 if bf16 else torch.float32
    shared = [n for n in RING if "agent" not in n]
    for step, K in enumerate([M, 40, M, 7, 1, 149, M, 64]):  # the 6th call wraps
        buf0, buf1 = (torch.rand((M, pitch or F), device="cuda", generator=g).to(dt) for _ in range(2))
        ast0, ast1 = (torch.rand((M, 2), device="cuda", generator=g) for _ in range(2))
        m0, m1 = (torch.rand((M, mem), device="cuda", generator=g) for _ in range(2))
        rot = torch.randint(-1, 2, (M,), device="cuda", generator=g).to(torch.int8)
        ph = torch.randint(0, 3, (M,), device="cuda", generator=g).to(torch.int8)
        rew = torch.randn((M,), device="cuda", generator=g)
        done = (torch.rand((E,), device="cuda", generator=g) < 0.4).to(torch.uint8)
        kw = dict(n_envs=E, n_ants=N, k=K, seed=99, step=step, env_id_base=2, obs_pitch=pitch)
        a.record_pre(buf0, ast0, None, rot, ph, **kw)
        a.record_post(buf1, ast1, None, rew, done)
        b.record_pre(buf0, ast0, m0, rot, ph, **kw)
        b.record_post(buf1, ast1, m1, rew, done)
        _same_rings(a, b, shared)
        assert torch.equal(a.agent_states, b.agent_states[:, :2]) and torch.equal(a.new_agent_states, b.new_agent_states[:, :2])
        idx = torch.from_numpy(R.sample_indices(99, step, 2, M, K)).cuda()
        _, rows, head = R.ring_rows((a.head - K) % Lr, Lr, K)  # K <= max_len here: every entry is written
        assert head == a.head
        rows = torch.from_numpy(rows).cuda()
        assert torch.equal(a.agent_states[rows], ast0[idx]) and torch.equal(a.new_agent_states[rows], ast1[idx])
    c, d = DeviceReplayMemory(100, P, [2], [2]), DeviceReplayMemory(100, P, [2 + mem], [2])
    c.head = d.head = 97
    c.record_pre(buf0, ast0, None, rot, None, n_envs=E, n_ants=N, obs_pitch=pitch)  # K = M > max_len; pheromone None: 1
    c.record_post(buf1, ast1, None, rew, done.bool())
    d.record_pre(buf0, ast0, m0, rot, None, n_envs=E, n_ants=N, obs_pitch=pitch)
    d.record_post(buf1, ast1, m1, rew, done.bool())
    _same_rings(c, d, shared)
    assert torch.equal(c.agent_states, d.agent_states[:, :2])


# ---- 3. the training step against the contract
def _host_state(tr):
    s = L.new_state({k: v.cpu() for k, v in tr.state_dict().items()})
    t = tr.target_state_dict()
    s["target_w3"], s["target_b3"] = t["layer3.weight"].cpu(), t["layer3.bias"].cpu()
    return s


@pytest.mark.parametrize("B", [1, 31, 264, 4096, 65536])
@pytest.mark.parametrize("with_done", [False, True])
def test_step_equals_the_contract(B, with_done):
    import torch
    from antsrl_amd.train import LinearTrainer
    F, N = 294, 3000
    tr = LinearTrainer(F, "cuda", seed=3 + B % 7)
    tr.target_l3.mul_(0.5)  # a target layer3 that differs from the model's
    arrays, g = _random_replay(N, F, B + with_done, with_done)
    idx = torch.randint(0, N, (B,), device="cuda", generator=g)
    assert tr.launches(B) == (1 if B <= 512 else 2)
    host = _host_state(tr)
    batch = tuple(a[idx].cpu().numpy() for a in arrays)
    loss_ref, g_ref = L.contract_train_step(host, batch, update=False)
    before = tr.state_dict()
    loss = float(tr.step(arrays, idx))
    gd = {k: v.cpu() for k, v in tr.grad_dict().items()}
    worst_g = max(float((gd[k] - g_ref[k]).abs().max() / g_ref[k].abs().max()) for k in L.TRAINED)
    rel_l = abs(loss - loss_ref) / abs(loss_ref)
    # Adam, from the gradient the device itself produced: the moments bit for bit, the parameters within 1e-4 of a step
    L.adam(host, gd)
    st, after = tr.adam_state(), tr.state_dict()
    worst_p = max(float((after[k].cpu() - host["sd"][k]).abs().max()) for k in L.TRAINED) / tr.lr
    print("\nB = %5d done %d: gradient %.3g of the tensor's max, loss %.3g relative, heads %.3g of a step of lr"
          % (B, with_done, worst_g, rel_l, worst_p))
    assert worst_g <= BOUND_GRAD[B > 4096] and rel_l <= BOUND_LOSS[B > 4096] and worst_p <= BOUND_HEADS
    for k in L.TRAINED:
        assert torch.equal(st["exp_avg"][k].cpu(), host["m"][k]) and torch.equal(st["exp_avg_sq"][k].cpu(), host["v"][k]), k
    for k in L.NAMES[:2]:
        assert torch.equal(after[k], before[k])
    # grad() then apply() on a twin gives the bits of step()
    tw = LinearTrainer(F, "cuda", seed=3 + B % 7)
    tw.target_l3.mul_(0.5)
    l2 = tw.grad(arrays, idx)
    tw.apply()

    def why():  # (built on a failure only) above 512 rows the workspace tells which workgroups and outputs differ
        if B <= 512:
            return "grad() %.10g against step() %.10g" % (float(l2), loss)
        return twin_report(linear_snapshot(tr, torch.tensor(loss), B), linear_snapshot(tw, l2, B))
    assert float(l2) == loss, why()
    assert torch.equal(tw.heads, tr.heads), why()
    assert torch.equal(tw._adam, tr._adam), why()
    assert torch.equal(tw.grads, tr.grads), why()


# ---- 4. against the fixture, in fp32
def _fixture_batch(fx, c):
    pos = np.searchsorted(fx["rows/index"], fx["c%d/idx" % c])
    return tuple(fx["rows/" + k][pos] for k in RING)


def test_step_against_the_references_recorded_run():
    import torch
    from antsrl_amd.train import LinearTrainer
    fx = np.load(PATH)
    tr = LinearTrainer(294, "cuda", state_dict={k: torch.from_numpy(fx["init/" + k]) for k in L.NAMES})
    assert list(tr.state_dict()) == list(L.NAMES)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    arrays = tuple(dev(fx["rows/" + k]) for k in RING)
    for c in range(3):
        idx = dev(np.searchsorted(fx["rows/index"], fx["c%d/idx" % c]).astype(np.int64))
        before = tr.state_dict()
        loss = float(tr.train_on(arrays, idx, bool(fx["c%d/done" % c])))
        after, gd = tr.state_dict(), tr.grad_dict()
        rel = abs(loss - float(fx["c%d/loss" % c])) / float(fx["c%d/loss" % c])
        cos_g = min(float(torch.nn.functional.cosine_similarity(gd[k].reshape(-1).cpu().double(),
                                                                 torch.from_numpy(fx["c%d/grad/%s" % (c, k)]).reshape(-1).double(), 0))
                    for k in L.TRAINED)
        cos_d = min(float(torch.nn.functional.cosine_similarity((after[k] - before[k]).reshape(-1).cpu().double(),
                                                                 torch.from_numpy(fx["c%d/delta/%s" % (c, k)]).reshape(-1).double(), 0))
                    for k in L.TRAINED)
        print("\ncall %d: loss %.6f (reference %.6f, relative %.3g), min cosine gradient %.6f, delta %.6f"
              % (c, loss, float(fx["c%d/loss" % c]), rel, cos_g, cos_d))
        # bfloat16 layer1 against the reference's fp32.  Measured on an MI355X over the three calls (the CPU restatement
        # gives the same figures): relative loss error 7.66e-5, 7.14e-5, 1.01e-4; 1 - cosine 2.0e-6 (gradients) and up to
        # 4.0e-5 (deltas: Adam's first steps are nearly sign(g), so one element near zero weighs more).  Bounds: 4 x.
        assert rel <= 4e-4 and 1.0 - cos_g <= 8e-6 and 1.0 - cos_d <= 1.6e-4
        teq = torch.equal(tr.target_l3, tr.heads[99:198])
        assert teq == bool(fx["c%d/target_eq_model" % c])
        for k in L.NAMES[:2]:
            assert torch.equal(after[k], before[k])


# ---- 5. determinism, the frozen layer1, zero gradients
def test_equal_inputs_equal_bits_and_layer1_is_never_written():
    import torch
    from antsrl_amd.train import LinearTrainer
    F, N = 294, 5000
    arrays, g = _random_replay(N, F, 11, True)
    arrays[2][:, 0] = torch.randint(0, 2, (N,), device="cuda", generator=g)  # rotation 2 is never taken: w2[2], b2[2] get zero gradients
    out = []
    for rep in range(2):
        tr = LinearTrainer(F, "cuda", seed=9)
        w1, b1 = tr.policy.w1.clone(), tr.policy.b1.clone()
        h0 = tr.heads.clone()
        gi = torch.Generator(device="cuda").manual_seed(4)
        losses = []
        for s in range(10):
            B = (264, 4096)[s % 2]
            losses.append(tr.step(arrays, torch.randint(0, N, (B,), device="cuda", generator=gi)).clone())
        assert torch.equal(tr.policy.w1, w1) and torch.equal(tr.policy.b1, b1)
        assert torch.equal(tr.heads[64:96], h0[64:96]) and torch.equal(tr.heads[98:99], h0[98:99])  # zero gradient: not moved
        assert not torch.equal(tr.heads[0:64], h0[0:64])
        out.append((torch.stack(losses), tr.heads.clone(), tr._adam.clone(), tr.grads.clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)


# ---- 6. acting
def test_get_action_against_the_recorded_actions():
    import torch
    from antsrl_amd.agent import CollectAgent
    fx = np.load(PATH)
    env = _env(E=1, N=64)  # supplies the shapes: one colony of 64 ants, 7 x 7 x 6 observations
    ag = CollectAgent()
    ag.setup(env)
    ag.trainer.load_state_dict({k: torch.from_numpy(fx["act/w/" + k]) for k in L.NAMES})
    w = {k: torch.from_numpy(fx["act/w/" + k]).double() for k in L.NAMES}
    left_out = total = 0
    for s in range(4):
        obs, ast = fx["act/s%d/obs" % s], fx["act/s%d/agent_state" % s]
        rot, ph = ag.get_action(obs, ast, False)
        x = torch.cat([torch.from_numpy(obs).reshape(64, -1), torch.from_numpy(ast)], 1).double()
        for head, got, want in ((0, rot.cpu().numpy() + 1, fx["act/s%d/rotation" % s] + 1),
                                (1, ph.cpu().numpy(), fx["act/s%d/pheromone" % s])):
            safe, _ = L.acting_gap_safe(w, x, head)  # the fp32 top-two gap against 4 sigma of the bfloat16 roundings
            assert np.array_equal(got[safe.numpy()], want[safe.numpy()])
            left_out += int((~safe).sum())
            total += 64
    print("\nacting: %d of %d decisions inside the bfloat16 bound (left out): %.2f %%" % (left_out, total, 100.0 * left_out / total))
    assert left_out <= 0.01 * total


# ---- 7. the loop
def _agent(**kw):
    from antsrl_amd.agent import CollectAgent
    return CollectAgent(epsilon=0.5, learning_rate=1e-3, min_replay=500, replay_size=3000, seed=7, **kw)


def _same_agents(a, b):
    import torch
    _same_rings(a.replay_memory, b.replay_memory)
    ta, tb = a.trainer, b.trainer
    assert torch.equal(ta.heads, tb.heads) and torch.equal(ta.target_l3, tb.target_l3) and torch.equal(ta._adam, tb._adam)
    assert (ta.step_count, ta.syncs) == (tb.step_count, tb.syncs)


def test_the_loop_equals_the_loop_driven_entry_by_entry():
    import torch
    from antsrl_amd.train import LinearTrainer
    steps, E, N = 36, 4, 64
    ag = _agent()
    r = drive_loop(ag, LinearTrainer, 264, True, lambda tr: torch.equal(tr.target_l3, tr.heads[99:198]), steps, E, N, max_time=12)
    tr, rm = r.trainer, r.ring
    assert len(rm) == min(3000, steps * E * N) and tr.step_count == steps - 1  # 256 rows after step 0: below min_replay
    assert r.synced_after_done and all(r.synced_after_done)
    for t, (x, y) in enumerate(zip(r.losses, r.host_losses)):
        assert (x == 0 and y == 0) or float(x) == float(y), "step %d" % t
    for t, ((r0, p0), (r1, p1)) in enumerate(zip(r.acts, r.host_acts)):
        assert torch.equal(r0, r1) and torch.equal(p0, p1), "actions, step %d" % t
    _same_rings(ag.replay_memory, rm)
    assert torch.equal(ag.trainer.heads, tr.heads) and torch.equal(ag.trainer._adam, tr._adam) and torch.equal(ag.trainer.target_l3, tr.target_l3)
    assert torch.equal(r.env_a.obs, r.env_b.obs)


def test_inloop_equals_standalone():
    import torch
    a, b = inloop_runs(_agent, True, steps=36, E=4, N=64, max_time=12)  # steps 0..9 stay below min_replay and do not train
    assert b.agent.inloop_hits >= 8 and a.agent.inloop_hits == 0  # the steps below min_replay took the observation kernel's actions
    for (r0, p0), (r1, p1) in zip(a.acts, b.acts):
        assert torch.equal(r0, r1) and torch.equal(p0, p1)
    for x, y in zip(a.losses, b.losses):
        assert (x == 0 and y == 0) or float(x) == float(y)
    _same_agents(a.agent, b.agent)
    assert torch.equal(a.env.obs, b.env.obs) and a.agent.trainer.step_count > 0


# ---- 8. learning happens
def test_the_loss_falls_on_one_minibatch():
    import torch
    from antsrl_amd.train import LinearTrainer
    arrays, g = _random_replay(2000, 294, 21, True)
    idx = torch.randint(0, 2000, (264,), device="cuda", generator=g)
    tr = LinearTrainer(294, "cuda", lr=1e-2, seed=1)
    # something a linear head can learn: every row ends its episode (y = reward) and the reward is linear in layer1's output
    st, ast, act, rw, nst, nast, dn = arrays
    h = torch.cat([st, ast], 1) @ tr.policy.w1.T + tr.policy.b1
    rw.copy_(h @ torch.randn((32,), device="cuda", generator=g))
    dn.fill_(True)
    t0 = tr.target_l3.clone()
    losses = [float(tr.step(arrays, idx)) for _ in range(400)]  # no sync: the target layer3 stays frozen
    assert torch.equal(tr.target_l3, t0)
    print("\nloss on one minibatch, 400 steps at lr 1e-2: %.5f -> %.5f" % (losses[0], losses[-1]))
    assert losses[-1] <= 0.1 * losses[0]


# ---- 9. the state_dict
def test_state_dict_names_and_the_save_load_round_trip(tmp_path):
    import torch
    from antsrl_amd.agent import CollectAgent
    env = _env()
    a, b = CollectAgent(seed=1), CollectAgent(seed=2)
    a.setup(env)
    b.setup(env)
    assert a.name == "collect_agent"
    sd = a.trainer.state_dict()
    assert list(sd) == ["explore_model.layer1.weight", "explore_model.layer1.bias", "explore_model.layer2.weight",
                        "explore_model.layer2.bias", "layer3.weight", "layer3.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(32, 296), (32,), (3, 32), (3,), (3, 32), (3,)]
    assert not torch.equal(b.trainer.heads, a.trainer.heads)
    path = str(tmp_path / "collect.h5")
    a.save_model(path)
    assert list(torch.load(path)) == list(sd)
    b.load_model(path)
    for k, v in b.trainer.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for k, v in b.trainer.target_state_dict().items():  # load_model sets the target net too
        assert torch.equal(v, sd[k]), k
    env.observe()
    ra, pa = (t.clone() for t in a.get_action(env.obs, env.agent_state, False, env=env))
    rb, pb = b.get_action(env.obs, env.agent_state, False, env=env)
    assert torch.equal(ra, rb) and torch.equal(pa, pb)
