"""The training step on the device (antsrl_memtrain_grad / antsrl_memtrain_apply, MemoryTrainer) against the comparators
of tests/memory_train_ref.py: `bf16_train_grads` (the kernels' precision contract, up to fp32 summation order),
`fp32_train_step` (the reference's arithmetic, pinned to the reference's own train() by
tests/test_memory_train_fixture.py) and `adam_step` / torch.optim.Adam.  The measured errors are printed (run with -s)
and recorded in DESIGN §7.7.

GRAD_TOL and LOSS_TOL here are measured, relative to each tensor's largest element, and against a comparator that runs
on the GPU itself: they hold the step to the reference's arithmetic end to end and no closer.  The sharp checks of the
kernels are in tests/test_gpu_memory_train_stages.py: inputs on which the step is exact in fp32 and must equal float64
bit for bit (gradients, loss, m, v, both bf16 packs), and every launch held element by element inside an a-priori bound
of float64 on its own inputs, at every width, seam and guard."""
import numpy as np
import pytest

from memory_train_ref import (TRAINED_KEYS, adam_step, bf16_train_grads, cosine, fixture_batch, fp32_train_step,
                              load_fixture)

pytestmark = pytest.mark.gpu

GRAD_TOL = 1.5e-2  # max |kernel - bf16_train_grads| / max |bf16_train_grads| per tensor: ~4x the largest measured (3.5e-3)
LOSS_TOL = 2e-6    # relative, kernel loss vs bf16_train_grads: ~4x the largest measured (5.2e-7)
MEMORY_HEAD = ("memory_layer1", "memory_layer2", "memory_layer3", "forget_layer")


def _trainer(sd=None, **kw):
    import torch
    from antsrl_amd.train import MemoryTrainer
    return MemoryTrainer(kw.pop("n_features", 294), torch.device("cuda"), state_dict=sd, **kw)


def _dev(batch):
    import torch
    return tuple(t.to("cuda").contiguous() for t in batch)


def _grad_err(tr, ref):
    got = tr.grad_dict()
    return {k: float((got[k] - ref[k]).abs().max() / ref[k].abs().max().clamp(min=1e-30)) for k in TRAINED_KEYS}


def _synth_batch(N, F, mem, seed, n_rot=3, n_ph=3, tail_reward=None):
    """Replay-like arrays with the value ranges of real transitions."""
    import torch
    g = torch.Generator().manual_seed(seed)
    st = (torch.rand((N, F), generator=g) < 0.3).float() * torch.rand((N, F), generator=g)
    ast = torch.cat([torch.rand((N, 2), generator=g) * 2 - 1, torch.rand((N, mem), generator=g) * 2 - 1], dim=1)
    act = torch.stack([torch.randint(0, n_rot, (N,), generator=g), torch.randint(0, n_ph, (N,), generator=g)], dim=1)
    rw = torch.randn((N,), generator=g)
    if tail_reward is not None:
        rw[-1] = tail_reward
    nst = (torch.rand((N, F), generator=g) < 0.3).float() * torch.rand((N, F), generator=g)
    nast = torch.cat([torch.rand((N, 2), generator=g) * 2 - 1, torch.rand((N, mem), generator=g) * 2 - 1], dim=1)
    dn = torch.rand((N,), generator=g) < 0.1
    return _dev((st, ast, act, rw, nst, nast, dn))


def test_against_the_reference_fixture():
    import torch
    sd, rec = load_fixture()
    tr = _trainer(sd, discount=float(rec["discount"]), lr=float(rec["lr"]))
    worst, worst_loss = 0.0, 0.0
    for c in range(3):
        batch = _dev(fixture_batch(rec, c))
        model, target = tr.state_dict(), tr.target_state_dict()
        loss = tr.grad(batch)
        bl, bg = bf16_train_grads(model, target, batch, float(rec["discount"]))
        fl, fg = fp32_train_step({k: v.cpu() for k, v in model.items()}, {k: v.cpu() for k, v in target.items()},
                                 fixture_batch(rec, c), float(rec["discount"]))
        err = _grad_err(tr, bg)
        lerr = abs(float(loss) - float(bl)) / abs(float(bl))
        cos = {k: cosine(tr.grad_dict()[k].cpu(), fg[k]) for k in TRAINED_KEYS}
        print("\ncall %d: loss %.6g (bf16 %.6g, fp32 %.6g, reference %.6g) | grad err vs bf16 max %.3g (%s) | "
              "cosine vs fp32 min %.5f" % (c, float(loss), float(bl), float(fl), float(rec["c%d/loss" % c]),
                                           max(err.values()), max(err, key=err.get), min(cos.values())))
        assert lerr <= LOSS_TOL, (c, lerr)
        assert max(err.values()) <= GRAD_TOL, (c, err)
        assert min(cos.values()) >= 0.99, (c, cos)
        assert abs(float(loss) - float(fl)) <= 1e-2 * abs(float(fl)), (c, float(loss), float(fl))
        worst, worst_loss = max(worst, max(err.values())), max(worst_loss, lerr)
        tr.apply()
        if bool(rec["c%d/done" % c]):
            tr.sync_target()
    print("fixture: worst grad err %.3g, worst loss err %.3g" % (worst, worst_loss))
    torch.cuda.synchronize()


def test_adam_stage_matches_torch():
    import torch
    tr = _trainer(seed=4, lr=1e-3)
    p0 = {k: v.clone() for k, v in tr.state_dict().items()}
    params = {k: torch.nn.Parameter(p0[k].clone()) for k in TRAINED_KEYS}
    opt = torch.optim.Adam([params[k] for k in TRAINED_KEYS], lr=1e-3, foreach=False)
    mine = {k: (p0[k].clone(), torch.zeros_like(p0[k]), torch.zeros_like(p0[k])) for k in TRAINED_KEYS}
    g = torch.Generator(device="cuda").manual_seed(5)
    zero = torch.rand(tr.trained_floats, device="cuda", generator=g) < 0.1  # never get a gradient
    worst_r, worst_t, worst_m, abs_r, abs_t = 0.0, 0.0, 0.0, 0.0, 0.0
    for s in range(1, 6):
        prev = tr.state_dict()
        flat = torch.randn(tr.trained_floats, device="cuda", generator=g) * 1e-2
        flat[zero] = 0.0
        tr.grads.copy_(flat)
        tr.apply()
        gd = tr.grad_dict(flat)
        for k in TRAINED_KEYS:
            params[k].grad = gd[k].clone()
            p, m, v = mine[k]
            mine[k] = adam_step(p, gd[k], m, v, s, 1e-3)
        opt.step()
        got = tr.state_dict()
        st = tr.adam_state()
        for k in TRAINED_KEYS:
            # ulp of the larger of |p| before and after the step (an update that crosses zero cancels p's own bits)
            ulp = torch.finfo(torch.float32).eps * torch.maximum(prev[k].abs(), got[k].abs()).clamp(min=1e-30)
            dr, dt = (got[k] - mine[k][0]).abs(), (got[k] - params[k].detach()).abs()
            worst_r = max(worst_r, float((dr / ulp).max()))
            worst_t = max(worst_t, float((dt / ulp).max()))
            abs_r, abs_t = max(abs_r, float(dr.max())), max(abs_t, float(dt.max()))
            if float((dr / ulp).max()) > 4:
                i = int((dr / ulp).reshape(-1).argmax())
                print("  step %d %s[%d]: before %.9g kernel %.9g restatement %.9g torch %.9g grad %.9g" % (
                    s, k, i, float(prev[k].reshape(-1)[i]), float(got[k].reshape(-1)[i]), float(mine[k][0].reshape(-1)[i]),
                    float(params[k].detach().reshape(-1)[i]), float(gd[k].reshape(-1)[i])))
            worst_m = max(worst_m, float((st["exp_avg"][k] - mine[k][1]).abs().max()),
                          float((st["exp_avg_sq"][k] - mine[k][2]).abs().max()))
    print("\nAdam, 5 steps at lr 1e-3: |kernel - restatement| max %.3g ulp of p (%.3g absolute; m, v: %.3g), "
          "|kernel - torch.optim.Adam(foreach=False)| max %.3g ulp of p (%.3g absolute)"
          % (worst_r, abs_r, worst_m, worst_t, abs_t))
    assert worst_m == 0.0  # Adam's moments: bit-identical to the restatement
    assert abs_r <= 1e-4 * 1e-3 and abs_t <= 1e-4 * 1e-3  # parameters: within 1e-4 of one step of lr
    flat_now = torch.cat([tr.state_dict()[k].reshape(-1) for k in TRAINED_KEYS])
    flat_0 = torch.cat([p0[k].reshape(-1) for k in TRAINED_KEYS])
    assert torch.equal(flat_now[zero], flat_0[zero])  # zero-gradient elements: bit-identical
    assert st["step"] == 5


def test_memory_head_is_never_touched():
    import torch
    tr = _trainer(seed=2, lr=1e-3)
    before = tr.state_dict()
    batch = _synth_batch(512, 294, 20, seed=1)
    for _ in range(10):
        tr.step(batch)
    after = tr.state_dict()
    for k in before:
        same = torch.equal(before[k], after[k])
        assert same == (k.split(".")[0] in MEMORY_HEAD), k
    assert set(tr.adam_state()["exp_avg"]) == set(TRAINED_KEYS)


def test_bit_identical_runs_and_idx_path():
    import torch
    N = 3000
    batch = _synth_batch(N, 294, 20, seed=3)
    idx = torch.randint(0, N, (1000,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    runs = []
    for _ in range(2):
        tr = _trainer(seed=6, lr=1e-3)
        losses = [tr.step(batch, idx).clone() for _ in range(3)]
        runs.append((torch.stack(losses), tr.grads.clone(), tr._model.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])  # masters, m, v and packs, padding included: byte for byte
    a, b = _trainer(seed=6), _trainer(seed=6)
    la = a.grad(batch, idx)
    lb = b.grad(tuple(t[idx].contiguous() for t in batch))
    assert torch.equal(la, lb) and torch.equal(a.grads, b.grads)


@pytest.mark.parametrize("power,mem", [(4, 10), (4, 20), (5, 10), (5, 20)])
def test_batch_sizes(power, mem):
    import torch
    errs = []
    for B in (1, 31, 32, 33, 264, 1000, 4097, 65536):
        # the last row's TD error dominates the gradient: a dropped or misplaced tail row would show
        batch = _synth_batch(B, 294, mem, seed=B, tail_reward=float(B))
        tr = _trainer(seed=B, power=power, mem_size=mem, discount=0.99)
        loss = tr.grad(batch)
        bl, bg = bf16_train_grads(tr.state_dict(), tr.target_state_dict(), batch, 0.99)
        err = max(_grad_err(tr, bg).values())
        lerr = abs(float(loss) - float(bl)) / abs(float(bl))
        errs.append((B, err, lerr))
        assert err <= GRAD_TOL and lerr <= LOSS_TOL, (B, err, lerr)
    print("\npower %d mem %d: (B, grad err, loss err) %s" % (power, mem, ["%d %.2g %.2g" % e for e in errs]))
    torch.cuda.synchronize()


def test_out_of_range_actions_contribute_nothing():
    import torch
    batch = list(_synth_batch(300, 294, 20, seed=9))
    act = batch[2].clone()
    act[::7, 0] = -1
    act[::5, 1] = 3
    act[::11, 0] = 99
    act[::13, 1] = -(1 << 40)
    batch[2] = act
    tr = _trainer(seed=1)
    loss = tr.grad(tuple(batch))
    bl, bg = bf16_train_grads(tr.state_dict(), tr.target_state_dict(), tuple(batch), 0.5)
    assert max(_grad_err(tr, bg).values()) <= GRAD_TOL and abs(float(loss) - float(bl)) <= LOSS_TOL * abs(float(bl))
    batch[2] = torch.full_like(act, 7)  # no valid action at all: exactly nothing
    loss = tr.grad(tuple(batch))
    assert float(loss) == 0.0 and not bool(tr.grads.any())


def test_policy_after_sync_acts_like_a_fresh_policy():
    import torch
    from antsrl_amd.policy import MemoryPolicy
    tr = _trainer(seed=3, lr=1e-3)
    batch = _synth_batch(264, 294, 20, seed=4)
    for _ in range(3):
        tr.step(batch)
    tr.sync_target()
    fresh = MemoryPolicy(294, torch.device("cuda"), seed=99)
    fresh.load_state_dict(tr.state_dict())
    g = torch.Generator(device="cpu").manual_seed(2)
    obs = torch.rand((1000, 7, 7, 6), generator=g).cuda()
    ast = (torch.rand((1000, 2), generator=g) * 2 - 1).cuda()
    mem = (torch.rand((1000, 20), generator=g) * 2 - 1).cuda()
    outs = []
    for pol in (tr.policy, fresh):
        q = torch.empty((1000, 6), device="cuda")
        out = torch.empty((1000, 20), device="cuda")
        r, p, m = pol.act(obs, ast, memory=mem, out=out, q=q)
        outs.append((r.clone(), p.clone(), m.clone(), q))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # the sync copied: training further does not move the policy's weights
    before = {k: v.clone() for k, v in tr.policy.params.items()}
    tr.step(batch)
    assert all(torch.equal(before[k], tr.policy.params[k]) for k in before)


def test_fit_a_fixed_minibatch():
    """Target frozen, one minibatch: the loss must fall at least 10x (sign or transpose errors would not)."""
    import torch
    tr = _trainer(seed=8, lr=1e-3, discount=0.99)
    batch = _synth_batch(264, 294, 20, seed=12)
    first = float(tr.grad(batch))
    losses = []
    for _ in range(300):
        losses.append(tr.step(batch))
    last = float(tr.grad(batch))
    print("\nfit: loss %.4g -> %.4g after 300 steps" % (first, last))
    assert last <= first / 10, (first, last)


def test_end_to_end_with_the_environment():
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.replay import DeviceReplayMemory
    from antsrl_amd.synth import random_actions, synth_init
    cfg = cm.make_cfg(4, 64, 64, 64, deposit_strength=256.0)
    env = BatchedAntsEnv(cfg)
    env.reset(synth_init(cfg, seed=5, n_food_discs=6, food_rmin=3, food_rmax=6))
    rot0, ph0 = random_actions(cfg, 1, seed=3)
    obs, ast, _, _ = env.step_update(rot0[0], ph0[0])
    P = tuple(obs.shape[-3:])
    F = int(np.prod(P))
    tr = _trainer(n_features=F, seed=1, discount=0.99, lr=1e-5)
    M = cfg.n_envs * cfg.n_ants
    replay = DeviceReplayMemory(20000, P, [22], [2], device=env.device)
    mem = torch.zeros((M, 20), device=env.device)
    nxt = torch.empty_like(mem)
    losses, dones, trained = [], [], 0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # no host read inside the loop
    try:
        for t in range(50):
            rot, ph, _ = tr.policy.act(obs, ast, memory=mem, out=nxt)
            o, a = obs.reshape(M, F).clone(), torch.cat([ast.reshape(M, 2), mem], dim=1)
            new_obs, new_ast, rew, done = env.step_update(rot, ph)
            replay.extend(o, a, (rot.reshape(-1).to(torch.int64) + 1, ph.reshape(-1)), rew.reshape(-1),
                          new_obs.reshape(M, F), torch.cat([new_ast.reshape(M, 2), nxt], dim=1), done)
            d = t % 10 == 9  # the episode boundary, known on the host
            before = tr.syncs
            loss = tr.train(replay, d, minibatch=264, min_replay=1000)
            if len(replay) >= 1000:
                trained += 1
                losses.append(loss)
                assert tr.syncs - before == (1 if d else 0), t
            mem, nxt = nxt, mem
            obs, ast = new_obs, new_ast
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ls = torch.stack(losses)
    assert trained >= 40 and bool(torch.isfinite(ls).all()), ls
    assert tr.syncs == sum(1 for t in range(50 - trained, 50) if t % 10 == 9)
    assert all(torch.equal(v, tr.target_state_dict()[k]) for k, v in tr.policy.params.items())
    print("\nend to end: %d training steps, loss %.4g -> %.4g, %d target syncs" % (trained, float(ls[0]), float(ls[-1]),
                                                                                  tr.syncs))
