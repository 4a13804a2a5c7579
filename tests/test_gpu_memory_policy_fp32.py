"""The memory agent net's fp32 mode on the device (MemoryPolicy(precision="fp32"), antsrl_policy_memory_ex with
ANTSRL_MEMNET_FP32) against `fp32_forward` (tests/memory_policy_ref.py), which test_memory_policy_fixture.py pins to
the reference's own classes.  The fp32 kernel is held to it up to fp32 summation order, and to the reference's recorded
actions.  The measured errors are printed (run with -s) and recorded in DESIGN §7.8."""
import ctypes as C

import numpy as np
import pytest

from memory_policy_ref import MODELS, fp32_forward, load_model, top2_margin

pytestmark = pytest.mark.gpu

Q_TOL = 8e-6    # |kernel - fp32_forward| <= Q_TOL * max(1, |q|): ~4x the largest error measured (2.0e-6 at c3)
MEM_TOL = 1e-6  # |kernel - fp32_forward| on the new memory: ~4x the largest error measured (2.1e-7)
DRIFT_TOL = 1e-6  # free-running fp32_forward memory after 40 env steps: ~4x the largest drift measured (1.8e-7)


def _policy(sd, device, precision="fp32", seed=0):
    from antsrl_amd.policy import MemoryPolicy, memnet_shape_from_state_dict
    shp = memnet_shape_from_state_dict(sd)
    pol = MemoryPolicy(shp["n_features"], device, power=shp["power"], mem_size=shp["mem_size"], n_rot=shp["n_rot"],
                       n_ph=shp["n_ph"], seed=seed, precision=precision)
    pol.load_state_dict(sd)
    return pol


def _run(pol, obs, ast, mem_in):
    import torch
    M = ast.reshape(-1, 2).shape[0]
    q = torch.empty((M, pol.n_rot + pol.n_ph), dtype=torch.float32, device=pol.device)
    out = torch.empty((M, pol.mem_size), dtype=torch.float32, device=pol.device)
    rot, ph, new = pol.act(obs, ast, memory=mem_in, out=out, q=q)
    return rot.reshape(-1).clone(), ph.reshape(-1).clone(), new, q


def _compare(pol, sd, obs, ast, mem_in, rot, ph, new, q, what, stats):
    """kernel vs fp32_forward: q and memory within the bounds; actions are the kernel's own q's argmax."""
    import torch
    fr, fp, fm = fp32_forward(sd, obs, ast, mem_in)
    fq = torch.cat([fr, fp], dim=1)
    eq = (q - fq).abs() / fq.abs().clamp(min=1.0)
    em = (new - fm).abs()
    assert float(eq.max()) <= Q_TOL, (what, float(eq.max()))
    assert float(em.max()) <= MEM_TOL, (what, float(em.max()))
    nr = pol.n_rot
    assert torch.equal(rot.long(), q[:, :nr].argmax(dim=1) - nr // 2) and torch.equal(ph.long(), q[:, nr:].argmax(dim=1))
    dis = int((rot.long() + nr // 2 != fr.argmax(dim=1)).sum()) + int((ph.long() != fp.argmax(dim=1)).sum())
    stats["q"].append(eq.reshape(-1))
    stats["mem"].append(em.reshape(-1))
    stats["dis"] += dis
    stats["rows"] += 2 * q.shape[0]


def _stats():
    return dict(q=[], mem=[], dis=0, rows=0)


def _report(name, stats):
    import torch
    q, m = torch.cat(stats["q"]), torch.cat(stats["mem"])
    print("\n%s: q rel err max %.3g | memory abs err max %.3g | fp32_forward action disagreements %d / %d"
          % (name, float(q.max()), float(m.max()), stats["dis"], stats["rows"]))


@pytest.mark.parametrize("model", MODELS)
def test_against_the_reference_fixture(model):
    """Both models' recorded steps; good_model's actions equal the reference's recorded ones wherever its own top-2
    margin is resolvable in fp32 (bf16 operands disagree on 48 / 1280 of them)."""
    import torch
    sd, rec = load_model(model)
    dev = torch.device("cuda")
    pol = _policy(sd, dev)
    stats = _stats()
    rec_dis = 0
    for t in range(rec["obs"].shape[0]):
        obs, ast, mem = (torch.from_numpy(rec[k][t]).to(dev) for k in ("obs", "agent_state", "mem_in"))
        rot, ph, new, q = _run(pol, obs, ast, mem)
        _compare(pol, sd, obs, ast, mem, rot, ph, new, q, (model, t), stats)
        for got, key, qkey in ((rot, "a_rot", "q_rot"), (ph, "a_ph", "q_ph")):
            want = torch.from_numpy(rec[key][t]).to(dev).long()
            rq = torch.from_numpy(rec[qkey][t]).to(dev)
            clear = top2_margin(rq) > 1e-4 * rq.abs().max(dim=1).values
            rec_dis += int((got.long() != want).sum())
            if model == "good_model":
                assert torch.equal(got.long()[clear], want[clear]), (model, t, key)
    _report(model, stats)
    print("%s: disagreements with the reference's recorded actions %d / %d" % (model, rec_dis, stats["rows"]))


@pytest.mark.parametrize("obs_dtype", ["float32", "bfloat16"])
def test_recurrence_through_the_environment(obs_dtype):
    """40 env steps driven by the fp32 kernel's actions, its memory carried in place; a free-running fp32_forward
    memory stays within DRIFT_TOL of it (the issue asks for 1e-4; bf16 operands drift 1.3e-3)."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    sd, _ = load_model("seeded_p5")
    cfg = cm.make_cfg(4, 64, 64, 64, deposit_strength=256.0)
    env = BatchedAntsEnv(cfg, obs_dtype=getattr(torch, obs_dtype))
    env.reset(synth_init(cfg, seed=5, n_food_discs=6, food_rmin=3, food_rmax=6))
    pol = _policy(sd, env.device)
    rot0, ph0 = random_actions(cfg, 1, seed=3)
    obs, ast, _, _ = env.step_update(rot0[0], ph0[0])
    free = torch.zeros((cfg.n_envs * cfg.n_ants, 20), device=env.device)
    stats = _stats()
    for t in range(40):
        mem_in = pol.memory.clone() if pol.memory is not None else torch.zeros_like(free)
        q = torch.empty((free.shape[0], 6), device=env.device)
        rot, ph, new = pol.act(obs, ast, q=q, env=env)
        assert new.data_ptr() == pol.memory.data_ptr()
        _compare(pol, sd, obs, ast, mem_in, rot.reshape(-1), ph.reshape(-1), new, q, t, stats)
        free = fp32_forward(sd, obs, ast, free)[2]
        obs, ast, _, _ = env.step_update(rot, ph)
    drift = float((free - pol.memory).abs().max())
    _report("env recurrence (%s obs)" % obs_dtype, stats)
    print("free-running fp32 memory drift after 40 steps: %.3g" % drift)
    assert np.isfinite(drift) and drift <= DRIFT_TOL


@pytest.mark.parametrize("F,power,mem,heads", [
    (296, 5, 2, 3),      # D = 300
    (298, 4, 20, 3),     # D = 320
    (299, 5, 20, 5),     # D = 321 (one padded tile past 320)
    (990, 5, 32, 1),     # D = 1024
    (294, 4, 1, 1),
    (294, 5, 10, 5),
    (294, 4, 32, 3),
])
def test_shapes(F, power, mem, heads):
    import torch
    from antsrl_amd.policy import MemoryPolicy
    dev = torch.device("cuda")
    pol = MemoryPolicy(F, dev, power=power, mem_size=mem, n_rot=heads, n_ph=heads, seed=F + power, precision="fp32")
    sd = {k: v.cpu() for k, v in pol.state_dict().items()}
    g = torch.Generator(device="cpu").manual_seed(F)
    M = 100
    obs = torch.rand((M, F), generator=g).to(dev).reshape(M, 1, 1, F)
    ast = torch.rand((M, 2), generator=g).to(dev)
    m0 = torch.rand((M, mem), generator=g).to(dev) * 2 - 1
    rot, ph, new, q = _run(pol, obs, ast, m0)
    assert q.shape == (M, 2 * heads)
    stats = _stats()
    _compare(pol, sd, obs, ast, m0, rot, ph, new, q, (F, power, mem, heads), stats)
    _report("shape F=%d power=%d mem=%d heads=%d" % (F, power, mem, heads), stats)
    assert int(rot.min()) >= -(heads // 2) and int(rot.max()) <= heads - 1 - heads // 2


def _c3_batch(model, steps=50):
    """good_model.h5 on a c3-shaped observation batch (1024 envs x 512 ants, 256 x 256, bf16 observations), aged
    `steps` steps with the fp32 kernel's own actions and carried memory."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    sd, _ = load_model(model)
    cfg = cm.make_cfg(1024, 512, 256, 256)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)
    env.reset(synth_init(cfg, seed=9))
    pol = _policy(sd, env.device)
    rot0, ph0 = random_actions(cfg, 1, seed=4)
    obs, ast, _, _ = env.step_update(rot0[0], ph0[0])
    for t in range(steps):
        rot, ph, _ = pol.act(obs, ast, env=env)
        obs, ast, _, _ = env.step_update(rot, ph)
    return sd, env, pol, obs, ast


def test_reference_checkpoint_at_c3_scale():
    """The shipped checkpoint's near-tied pheromone head: bf16 operands flip 6.85 % of its actions at c3 (DESIGN
    §7.6); fp32 operands must agree with fp32_forward on all but 1e-4 of them.  Also: a few ants of the c3 batch,
    run alone and in a batch of 100, give the same outputs bit for bit."""
    import torch
    sd, env, pol, obs, ast = _c3_batch("good_model")
    mem_in = pol.memory.clone()
    M = mem_in.shape[0]
    q = torch.empty((M, pol.n_rot + pol.n_ph), device=env.device)
    rot, ph, new = pol.act(obs, ast, q=q, env=env)
    rot, ph = rot.reshape(-1).long(), ph.reshape(-1).long()
    fr, fp, fm = fp32_forward(sd, obs, ast, mem_in)
    dr, dp = int((rot + 1 != fr.argmax(dim=1)).sum()), int((ph != fp.argmax(dim=1)).sum())
    rate = (dr + dp) / (2 * M)
    fq = torch.cat([fr, fp], dim=1)
    eq = float(((q - fq).abs() / fq.abs().clamp(min=1.0)).max())
    em = float((new - fm).abs().max())
    print("\nc3-scale good_model fp32 (%d ants): action disagreement vs fp32_forward %.3g (rotation %d, pheromone %d); "
          "q rel err max %.3g; memory max |kernel - fp32| %.3g" % (M, rate, dr, dp, eq, em))
    assert rate <= 1e-4
    assert eq <= Q_TOL and em <= MEM_TOL
    # batch invariance at c3: ants at the start, middle and end of the batch alone, and in a batch of 100
    o2, a2 = obs.reshape((M,) + tuple(obs.shape[-3:])), ast.reshape(M, 2)
    for i in (0, 31, 262143, M - 100, M - 1):
        for n in (1, 100):
            lo = min(i, M - n)
            r_, p_, m_, q_ = _run(pol, o2[lo:lo + n].contiguous(), a2[lo:lo + n].contiguous(), mem_in[lo:lo + n].contiguous())
            assert torch.equal(m_, new[lo:lo + n]) and torch.equal(q_, q[lo:lo + n]), (i, n)
            assert torch.equal(r_, rot[lo:lo + n].to(torch.int8)) and torch.equal(p_, ph[lo:lo + n].to(torch.int8)), (i, n)


def test_bit_exact_properties():
    import torch
    from antsrl_amd.policy import MemoryPolicy
    dev = torch.device("cuda")
    pol = MemoryPolicy(294, dev, power=5, mem_size=20, seed=7, precision="fp32")
    g = torch.Generator(device="cpu").manual_seed(1)
    M = 4097
    obs = torch.rand((M, 7, 7, 6), generator=g).to(dev)
    obs16 = obs.to(torch.bfloat16)
    obs_r = obs16.to(torch.float32).contiguous()  # bf16-representable float32
    ast = torch.rand((M, 2), generator=g).to(dev) * 5
    mem = (torch.rand((M, 20), generator=g).to(dev) - 0.5)
    r1, p1, m1, q1 = _run(pol, obs_r, ast, mem)
    # in place == out of place
    buf = mem.clone()
    qi = torch.empty_like(q1)
    ri, pi, mi = pol.act(obs_r, ast, memory=buf, q=qi)
    assert mi.data_ptr() == buf.data_ptr()
    assert torch.equal(mi, m1) and torch.equal(qi, q1) and torch.equal(ri, r1) and torch.equal(pi, p1)
    # bf16 observations == their exact float32 widening
    r2, p2, m2, q2 = _run(pol, obs16, ast, mem)
    assert torch.equal(m2, m1) and torch.equal(q2, q1) and torch.equal(r2, r1) and torch.equal(p2, p1)
    # deterministic
    r3, p3, m3, q3 = _run(pol, obs_r, ast, mem)
    assert torch.equal(m3, m1) and torch.equal(q3, q1)
    # no work crosses ants
    for n in (1, 31, 33, 100, 1000, 4097):
        rn, pn, mn, qn = _run(pol, obs_r[:n].contiguous(), ast[:n].contiguous(), mem[:n].contiguous())
        assert torch.equal(mn, m1[:n]) and torch.equal(qn, q1[:n]) and torch.equal(rn, r1[:n]), n
    for i in (0, 31, 32, 999, 4096):
        ri_, pi_, mi_, qi_ = _run(pol, obs_r[i:i + 1].contiguous(), ast[i:i + 1].contiguous(), mem[i:i + 1].contiguous())
        assert torch.equal(mi_, m1[i:i + 1]) and torch.equal(qi_, q1[i:i + 1]), i
    # the bf16 kernel is a different computation: the fp32 one must not be it
    r5, p5, m5, q5 = _run(MemoryPolicy(294, dev, power=5, mem_size=20, seed=7), obs_r, ast, mem)
    assert not torch.equal(q5, q1)


@pytest.mark.parametrize("model", MODELS)
def test_carried_memory_is_never_rounded(model):
    """forget_layer's bias at -1e4: s = 0, and the old memory comes back bit for bit, in place and out of place."""
    import torch
    sd, rec = load_model(model)
    dev = torch.device("cuda")
    obs, ast = (torch.from_numpy(rec[k][3]).to(dev) for k in ("obs", "agent_state"))
    M = ast.shape[0]
    mem = (torch.rand((M, sd["memory_layer3.weight"].shape[0]), generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev)
    assert float((mem.to(torch.bfloat16).float() != mem).float().mean()) > 0.99  # not bf16-representable
    sd2 = dict(sd)
    sd2["forget_layer.bias"] = torch.full_like(sd["forget_layer.bias"], -1e4)
    pol = _policy(sd2, dev)
    rot, ph, new, q = _run(pol, obs, ast, mem)
    assert torch.equal(new, mem)
    buf = mem.clone()
    pol.act(obs, ast, memory=buf)
    assert torch.equal(buf, mem)


def test_default_is_unchanged():
    """MemoryPolicy() is bf16, bit for bit; antsrl_policy_memory_ex(BF16) == antsrl_policy_memory, bit for bit."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.policy import MemoryPolicy
    sd, rec = load_model("good_model")
    dev = torch.device("cuda")
    a = _policy(sd, dev, precision="bf16")
    from antsrl_amd.policy import memnet_shape_from_state_dict
    shp = memnet_shape_from_state_dict(sd)
    b = MemoryPolicy(294, dev, power=shp["power"], mem_size=shp["mem_size"])
    b.load_state_dict(sd)
    assert a.precision == b.precision == "bf16"
    obs, ast, mem = (torch.from_numpy(rec[k][5]).to(dev) for k in ("obs", "agent_state", "mem_in"))
    ra, pa, ma, qa = _run(a, obs, ast, mem)
    rb, pb, mb, qb = _run(b, obs, ast, mem)
    assert torch.equal(ra, rb) and torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(qa, qb)
    # the old entry point on the same packed weights
    lib = _lib.load()
    M = ast.shape[0]
    q = torch.empty_like(qa)
    out = torch.empty_like(ma)
    rot = torch.empty((M,), dtype=torch.int8, device=dev)
    ph = torch.empty_like(rot)

    def p(t):
        return C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    _lib.check(lib.antsrl_policy_memory(C.byref(b.shape), p(b.packed), p(obs), 0, p(ast), p(mem), M, p(out), p(rot), p(ph),
                                        p(q), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "policy_memory")
    assert torch.equal(rot, ra) and torch.equal(ph, pa) and torch.equal(out, ma) and torch.equal(q, qa)


def test_trainer_acts_in_fp32_after_sync():
    """MemoryTrainer(policy_precision="fp32"): after training steps and sync_target(), its policy equals a fresh fp32
    MemoryPolicy loaded with target_state_dict(), bit for bit (and differs from a bf16 one)."""
    import torch
    from antsrl_amd.policy import MemoryPolicy
    from antsrl_amd.train import MemoryTrainer
    dev = torch.device("cuda")
    tr = MemoryTrainer(294, dev, power=4, mem_size=10, lr=1e-3, seed=11, policy_precision="fp32")
    assert tr.policy.precision == "fp32"
    g = torch.Generator(device="cpu").manual_seed(5)
    B, F, A = 264, 294, 2 + 10
    batch = (torch.rand((B, 7, 7, 6), generator=g).to(dev), (torch.rand((B, A), generator=g) * 2 - 1).to(dev),
             torch.randint(0, 3, (B, 2), generator=g).to(dev), torch.rand((B,), generator=g).to(dev),
             torch.rand((B, 7, 7, 6), generator=g).to(dev), (torch.rand((B, A), generator=g) * 2 - 1).to(dev),
             torch.zeros((B,), dtype=torch.bool, device=dev))
    before = tr.target_state_dict()
    for _ in range(3):
        tr.step(batch)
    tr.sync_target()
    assert not torch.equal(tr.target_state_dict()["layer1.weight"], before["layer1.weight"])  # the sync moved weights
    ref = MemoryPolicy(294, dev, power=4, mem_size=10, precision="fp32")
    ref.load_state_dict(tr.target_state_dict())
    M = 1000
    obs = torch.rand((M, 7, 7, 6), generator=g).to(dev)
    ast = torch.rand((M, 2), generator=g).to(dev)
    mem = torch.rand((M, 10), generator=g).to(dev) * 2 - 1
    r1, p1, m1, q1 = _run(tr.policy, obs, ast, mem)
    r2, p2, m2, q2 = _run(ref, obs, ast, mem)
    assert torch.equal(r1, r2) and torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(q1, q2)
    bf = MemoryPolicy(294, dev, power=4, mem_size=10)
    bf.load_state_dict(tr.target_state_dict())
    assert not torch.equal(_run(bf, obs, ast, mem)[3], q1)
