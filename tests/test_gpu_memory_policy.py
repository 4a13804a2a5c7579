"""The memory agent net on the device (antsrl_policy_memory, bf16 MFMA) against the comparators of
tests/memory_policy_ref.py: `bf16_forward` (the kernel's precision contract, up to fp32 summation order) and
`fp32_forward` (the reference's precision, pinned to the reference's own classes by tests/test_memory_policy_fixture.py).
The measured errors are printed (run with -s) and recorded in DESIGN §7."""
import numpy as np
import pytest

from memory_policy_ref import MODELS, bf16_forward, fp32_forward, load_model, top2_margin

pytestmark = pytest.mark.gpu

Q_TOL = 2.5e-3    # |kernel - bf16_forward| <= Q_TOL * max(1, |q|): ~4x the largest error measured (6.0e-4)
MEM_TOL = 2e-3    # |kernel - bf16_forward| on the new memory: ~4x the largest error measured (4.4e-4)
MARGIN = 0.05     # rows whose fp32 top-2 margin exceeds max(MARGIN, MARGIN_REL * max |q| of the row) must pick the fp32
MARGIN_REL = 1e-2  # action: the shipped checkpoint's q values are O(100-300), and bf16 operands alone move them by up to
                   # 0.7 there (2.8e-3 relative, tests/test_memory_policy_fixture.py's bf16-vs-fp32 comparison)


def _policy(sd, device, seed=0):
    from antsrl_amd.policy import MemoryPolicy, memnet_shape_from_state_dict
    shp = memnet_shape_from_state_dict(sd)
    pol = MemoryPolicy(shp["n_features"], device, power=shp["power"], mem_size=shp["mem_size"], n_rot=shp["n_rot"],
                       n_ph=shp["n_ph"], seed=seed)
    pol.load_state_dict(sd)
    return pol


def _run(pol, obs, ast, mem_in):
    import torch
    M = ast.reshape(-1, 2).shape[0]
    q = torch.empty((M, pol.n_rot + pol.n_ph), dtype=torch.float32, device=pol.device)
    out = torch.empty((M, pol.mem_size), dtype=torch.float32, device=pol.device)
    rot, ph, new = pol.act(obs, ast, memory=mem_in, out=out, q=q)
    return rot.reshape(-1).clone(), ph.reshape(-1).clone(), new, q


def _compare(pol, sd, obs, ast, mem_in, rot, ph, new, q, what, stats=None):
    """kernel vs bf16_forward (asserted) and vs fp32_forward (actions on clear rows)."""
    import torch
    br, bp, bm = bf16_forward(sd, obs, ast, mem_in)
    bq = torch.cat([br, bp], dim=1)
    eq = ((q - bq).abs() / bq.abs().clamp(min=1.0))
    em = (new - bm).abs()
    assert float(eq.max()) <= Q_TOL, (what, float(eq.max()))
    assert float(em.max()) <= MEM_TOL, (what, float(em.max()))
    fr, fp, fm = fp32_forward(sd, obs, ast, mem_in)
    nr = pol.n_rot
    assert torch.equal(rot.long(), q[:, :nr].argmax(dim=1) - nr // 2) and torch.equal(ph.long(), q[:, nr:].argmax(dim=1))
    dis = 0
    for head, act in ((fr, rot.long() + nr // 2), (fp, ph.long())):
        clear = top2_margin(head) > torch.clamp(MARGIN_REL * head.abs().max(dim=1).values, min=MARGIN)
        assert torch.equal(act[clear], head.argmax(dim=1)[clear]), what
        dis += int((act != head.argmax(dim=1)).sum())
    if stats is not None:
        stats["q"].append(eq.reshape(-1))
        stats["mem"].append(em.reshape(-1))
        stats["dis"] += dis
        stats["rows"] += 2 * q.shape[0]
    return dis


def _report(name, stats):
    import torch
    q, m = torch.cat(stats["q"]), torch.cat(stats["mem"])
    print("\n%s: q rel err max %.3g p99.9 %.3g | memory abs err max %.3g p99.9 %.3g | fp32 action disagreements %d / %d"
          % (name, float(q.max()), float(q.quantile(0.999)), float(m.max()), float(m.quantile(0.999)), stats["dis"], stats["rows"]))


@pytest.mark.parametrize("model", MODELS)
def test_against_the_reference_fixture(model):
    import torch
    sd, rec = load_model(model)
    dev = torch.device("cuda")
    pol = _policy(sd, dev)
    stats = dict(q=[], mem=[], dis=0, rows=0)
    for t in range(rec["obs"].shape[0]):
        obs, ast, mem = (torch.from_numpy(rec[k][t]).to(dev) for k in ("obs", "agent_state", "mem_in"))
        rot, ph, new, q = _run(pol, obs, ast, mem)
        _compare(pol, sd, obs, ast, mem, rot, ph, new, q, (model, t), stats)
    _report(model, stats)


@pytest.mark.parametrize("obs_dtype", ["float32", "bfloat16"])
def test_recurrence_through_the_environment(obs_dtype):
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
    free = torch.zeros((cfg.n_envs * cfg.n_ants, 20), device=env.device)  # fp32_forward carrying its own memory
    stats = dict(q=[], mem=[], dis=0, rows=0)
    for t in range(40):
        mem_in = pol.memory.clone() if pol.memory is not None else torch.zeros_like(free)
        q = torch.empty((free.shape[0], 6), device=env.device)
        rot, ph, new = pol.act(obs, ast, q=q, env=env)  # in place on pol.memory
        assert new.data_ptr() == pol.memory.data_ptr()
        _compare(pol, sd, obs, ast, mem_in, rot.reshape(-1), ph.reshape(-1), new, q, t, stats)
        free = fp32_forward(sd, obs, ast, free)[2]
        obs, ast, _, _ = env.step_update(rot, ph)  # the kernel's actions drive the env
    drift = float((free - pol.memory).abs().max())
    _report("env recurrence (%s obs)" % obs_dtype, stats)
    print("free-running fp32 memory drift after 40 steps: %.3g" % drift)
    assert np.isfinite(drift) and drift <= 0.1


def test_bit_exact_properties():
    import torch
    from antsrl_amd.policy import MemoryPolicy
    dev = torch.device("cuda")
    pol = MemoryPolicy(294, dev, power=5, mem_size=20, seed=7)
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
    # bf16 observations == their float32 widening
    r2, p2, m2, q2 = _run(pol, obs16, ast, mem)
    assert torch.equal(m2, m1) and torch.equal(q2, q1) and torch.equal(r2, r1) and torch.equal(p2, p1)
    # deterministic
    r3, p3, m3, q3 = _run(pol, obs_r, ast, mem)
    assert torch.equal(m3, m1) and torch.equal(q3, q1)
    # no work crosses ants: row i of a batch of n == the same ant alone, for batches of several sizes
    for n in (1, 31, 33, 1000, 4097):
        rn, pn, mn, qn = _run(pol, obs_r[:n].contiguous(), ast[:n].contiguous(), mem[:n].contiguous())
        assert torch.equal(mn, m1[:n]) and torch.equal(qn, q1[:n]) and torch.equal(rn, r1[:n]), n
    for i in (0, 31, 32, 999, 4096):
        ri_, pi_, mi_, qi_ = _run(pol, obs_r[i:i + 1].contiguous(), ast[i:i + 1].contiguous(), mem[i:i + 1].contiguous())
        assert torch.equal(mi_, m1[i:i + 1]) and torch.equal(qi_, q1[i:i + 1]), i


@pytest.mark.parametrize("model", MODELS)
def test_carried_memory_is_never_rounded(model):
    """With forget_layer's bias at -1e4, s = sigmoid(...) is exactly 0 and new_memory = old_memory * 1 must come back
    bit for bit: old values that bf16 cannot represent would lose their low 16 bits if the carried memory were rounded
    anywhere (read, blend or write).  With +1e4, s = 1 and the new memory is tanh(M3 m) alone: equal to bf16_forward's
    to the contract's tolerance (no trace of the old memory's blend)."""
    import torch
    sd, rec = load_model(model)
    dev = torch.device("cuda")
    obs, ast = (torch.from_numpy(rec[k][3]).to(dev) for k in ("obs", "agent_state"))
    M = ast.shape[0]
    mem = (torch.rand((M, sd["memory_layer3.weight"].shape[0]), generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev)
    assert float((mem.to(torch.bfloat16).float() != mem).float().mean()) > 0.99  # not bf16-representable
    for bias, want_old in ((-1e4, True), (1e4, False)):
        sd2 = dict(sd)
        sd2["forget_layer.bias"] = torch.full_like(sd["forget_layer.bias"], bias)
        pol = _policy(sd2, dev)
        rot, ph, new, q = _run(pol, obs, ast, mem)
        if want_old:
            assert torch.equal(new, mem)
        else:
            bm = bf16_forward(sd2, obs, ast, mem)[2]
            assert float((new - bm).abs().max()) <= MEM_TOL
        # in place: the same, bit for bit
        buf = mem.clone()
        pol.act(obs, ast, memory=buf)
        assert torch.equal(buf, new)


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
    pol = MemoryPolicy(F, dev, power=power, mem_size=mem, n_rot=heads, n_ph=heads, seed=F + power)
    sd = {k: v.cpu() for k, v in pol.state_dict().items()}
    g = torch.Generator(device="cpu").manual_seed(F)
    M = 100
    obs = torch.rand((M, F), generator=g).to(dev).reshape(M, 1, 1, F)
    ast = torch.rand((M, 2), generator=g).to(dev)
    m0 = torch.rand((M, mem), generator=g).to(dev) * 2 - 1
    rot, ph, new, q = _run(pol, obs, ast, m0)
    assert q.shape == (M, 2 * heads)
    stats = dict(q=[], mem=[], dis=0, rows=0)
    _compare(pol, sd, obs, ast, m0, rot, ph, new, q, (F, power, mem, heads), stats)
    _report("shape F=%d power=%d mem=%d heads=%d" % (F, power, mem, heads), stats)
    assert int(rot.min()) >= -(heads // 2) and int(rot.max()) <= heads - 1 - heads // 2


def test_reference_checkpoint_at_c3_scale():
    """good_model.h5's weights on a full c3-shaped observation batch (1024 envs x 512 ants, 256 x 256, the generator's
    6 channels), aged 50 steps with the kernel's own actions and carried memory."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import random_actions, synth_init
    sd, _ = load_model("good_model")
    cfg = cm.make_cfg(1024, 512, 256, 256)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)
    env.reset(synth_init(cfg, seed=9))
    pol = _policy(sd, env.device)
    rot0, ph0 = random_actions(cfg, 1, seed=4)
    obs, ast, _, _ = env.step_update(rot0[0], ph0[0])
    for t in range(50):
        rot, ph, _ = pol.act(obs, ast, env=env)
        obs, ast, _, _ = env.step_update(rot, ph)
    mem_in = pol.memory.clone()
    rot, ph, new = pol.act(obs, ast, env=env)
    rot, ph = rot.reshape(-1).long(), ph.reshape(-1).long()
    fr, fp, fm = fp32_forward(sd, obs, ast, mem_in)
    br, bp, bm = bf16_forward(sd, obs, ast, mem_in)
    M = fr.shape[0]

    def rate(a_r, a_p, ref_r, ref_p):
        return float(((a_r != ref_r).sum() + (a_p != ref_p).sum())) / (2 * M)
    k_f = rate(rot + 1, ph, fr.argmax(dim=1), fp.argmax(dim=1))
    b_f = rate(br.argmax(dim=1), bp.argmax(dim=1), fr.argmax(dim=1), fp.argmax(dim=1))
    k_b = rate(rot + 1, ph, br.argmax(dim=1), bp.argmax(dim=1))
    print("\nc3-scale good_model (%d ants): action disagreement kernel vs fp32 %.3g (rotation %.3g, pheromone %.3g); "
          "bf16_forward vs fp32 %.3g; kernel vs bf16_forward %.3g; memory max |kernel - fp32| %.3g"
          % (M, k_f, float((rot + 1 != fr.argmax(dim=1)).float().mean()), float((ph != fp.argmax(dim=1)).float().mean()),
             b_f, k_b, float((new - fm).abs().max())))
    # This checkpoint's pheromone q values are near-tied (margins of ~0.1 on values of ~70), so bf16 operands alone flip
    # several % of its actions against fp32: the kernel is held to the bf16 contract's own rate, and to
    # bf16_forward up to fp32 summation order.
    assert k_b <= 2e-3
    assert k_f <= 1.1 * b_f + 1e-3
    assert float((new - bm).abs().max()) <= MEM_TOL
