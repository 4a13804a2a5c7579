"""In-loop policy inference (antsrl_policy_mlp, bf16 MFMA) against a plain PyTorch fp32 reference of
the same linear net on the same bf16-rounded operands."""
import numpy as np
import pytest

from policy_ref import bf16_logits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("E,N,R", [(3, 50, 0), (4, 64, 2), (1, 1, 0)])
def test_policy_matches_torch_reference(E, N, R):
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.policy import LinearPolicy
    from antsrl_amd.synth import synth_init
    cfg = cm.make_cfg(E, N, 64, 64, n_rocks=R, deposit_strength=256.0)
    env = BatchedAntsEnv(cfg)
    env.reset(synth_init(cfg, seed=3, n_food_discs=6, food_rmin=3, food_rmax=6))
    pol = LinearPolicy(49 * cfg.n_channels, env.device, seed=1)
    rng = np.random.default_rng(0)
    for t in range(4):
        obs, ast, rew, done = env.step_update(rng.integers(-1, 2, (E, N), dtype=np.int8),
                                              rng.integers(0, 3, (E, N), dtype=np.int8))
        logits = torch.empty((E * N, 6), dtype=torch.float32, device=env.device)
        rot, ph = pol.act(obs, ast, logits)
        ref = bf16_logits(pol, obs, ast)
        # fp32 accumulation order differs (MFMA k-chains vs GEMM): tight absolute tolerance on O(1) logits
        assert torch.allclose(logits, ref, rtol=0, atol=2e-3), float((logits - ref).abs().max())
        # actions: equal to the reference argmax wherever its top-2 margin exceeds the tolerance
        for head, act, off in ((ref[:, :3], rot.reshape(-1) + 1, 0), (ref[:, 3:], ph.reshape(-1), 0)):
            top2 = head.topk(2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > 4e-3
            assert torch.equal(act[clear].long(), head.argmax(dim=1)[clear])
        assert rot.shape == (E, N) and rot.dtype == torch.int8 and int(rot.min()) >= -1 and int(rot.max()) <= 1
        assert int(ph.min()) >= 0 and int(ph.max()) <= 2
    # the actions drive the next step directly (config 5's loop)
    obs, ast, rew, done = env.step_update(rot, ph)


def test_policy_rotation_only_head():
    import torch
    from antsrl_amd.policy import LinearPolicy
    dev = torch.device("cuda")
    pol = LinearPolicy(49 * 6, dev, with_pheromone_head=False, seed=2)
    obs = torch.rand((70, 7, 7, 6), device=dev)
    ast = torch.rand((70, 2), device=dev)
    rot, ph = pol.act(obs, ast)
    assert ph is None and rot.shape == (70,)
    ref = bf16_logits(pol, obs, ast)
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 4e-3
    assert torch.equal((rot + 1)[clear].long(), ref.argmax(dim=1)[clear])


def test_policy_on_bfloat16_observations_matches_float32_path():
    """A bf16 observation tensor (antsrl_set_obs_format) is what the policy rounds its float32 input
    to: actions and logits are identical on both paths."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.policy import LinearPolicy
    from antsrl_amd.synth import random_actions, synth_init
    for R in (0, 3):
        cfg = cm.make_cfg(3, 200, 64, 64, n_rocks=R, deposit_strength=256.0)
        init = synth_init(cfg, seed=8, n_food_discs=5, food_rmin=2, food_rmax=5)
        a, b = BatchedAntsEnv(cfg), BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)
        a.reset(init)
        b.reset(init)
        rot, ph = random_actions(cfg, 3, seed=2)
        for t in range(3):
            a.step_update(rot[t], ph[t], None)
            b.step_update(rot[t], ph[t], None)
        pol = LinearPolicy(cfg.pside * cfg.pside * cfg.n_channels, a.device, seed=4)
        la = torch.empty((3 * 200, 6), device=a.device)
        lb = torch.empty_like(la)
        ra, pa = pol.act(a.obs, a.agent_state, logits=la)
        ra, pa = ra.clone(), pa.clone()
        rb, pb = pol.act(b.obs, b.agent_state, logits=lb, env=b)
        assert torch.equal(la, lb) and torch.equal(ra, rb) and torch.equal(pa, pb)


@pytest.mark.parametrize("F", [4, 9, 62, 63, 64, 65, 66, 127, 128, 130, 343, 894, 895, 896, 958, 1000, 1022])
def test_policy_feature_sizes_and_row_counts(F):
    """Chunk boundaries of the streamed rows: feature counts around multiples of 64 (whole chunks, a
    partial last chunk, the two agent_state inputs alone in the last chunk), row counts that are not a
    multiple of the 32-ant tile, float32 and bfloat16 observations.  F > 848 takes the chunked kernel (k_policy_mlp: the
    flat kernel's LDS image no longer fits), 894 .. 1022 on and around its chunk boundaries."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.policy import LinearPolicy
    dev = torch.device("cuda")
    henv = BatchedAntsEnv(cm.make_cfg(1, 4, 16, 16), obs_dtype=torch.bfloat16)  # only supplies the bf16 handle
    pol = LinearPolicy(F, dev, seed=F)
    g = torch.Generator(device=dev)
    g.manual_seed(F)
    for M in (1, 31, 33, 100):
        obs = torch.rand((M, F), device=dev, generator=g) * 2 - 1
        ast = torch.rand((M, 2), device=dev, generator=g) * 5
        ref = bf16_logits(pol, obs, ast)
        l32 = torch.empty((M, 6), device=dev)
        l16 = torch.empty((M, 6), device=dev)
        r32, p32 = pol.act(obs.view(M, 1, 1, F), ast, logits=l32)
        r32, p32 = r32.clone(), p32.clone()
        r16, p16 = pol.act(obs.to(torch.bfloat16).view(M, 1, 1, F), ast, logits=l16, env=henv)
        assert torch.allclose(l32, ref, rtol=0, atol=3e-3 * max(1.0, (F / 300) ** 0.5)), (F, M, float((l32 - ref).abs().max()))
        assert torch.equal(l32, l16) and torch.equal(r32, r16) and torch.equal(p32, p16), (F, M)


def test_full_config5_shard_policy_in_loop():
    """The FULL per-GPU shard of BASELINE config 5 (512 envs x 512 ants, 256x256, bfloat16 observations,
    the linear DQN net evaluated in the loop): every step's logits against the PyTorch reference of the
    same net over the whole batch, and three sampled environments against the oracle driven by the SAME
    actions (the policy's), observation rounded to bfloat16."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.policy import LinearPolicy
    from antsrl_amd.synth import synth_init
    from oracle.oracle import Oracle
    E, N, steps, pick = 512, 512, 4, [0, 255, 511]
    cfg = cm.make_cfg(E, N, 256, 256, deposit_strength=256.0)
    cfg_s = cm.make_cfg(len(pick), N, 256, 256, deposit_strength=256.0)
    init = synth_init(cfg, seed=55)
    orc = Oracle(cfg_s, {k: np.ascontiguousarray(v[pick]) for k, v in init.items()}, n_threads=3)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)
    env.reset(init)
    pol = LinearPolicy(cfg.pside * cfg.pside * cfg.n_channels, env.device, seed=5)
    env.observe()
    o_obs, o_ast, _ = orc.observe()
    rng = np.random.default_rng(8)
    logits = torch.empty((E * N, 6), dtype=torch.float32, device=env.device)
    for t in range(steps):
        # what the oracle saw is what the policy reads, rounded to bfloat16
        got = env.obs[pick].to(torch.float32).cpu().numpy()
        want = torch.from_numpy(o_obs.astype(np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
        ints = [0, 3, 4, 5]
        np.testing.assert_array_equal(got[..., ints], want[..., ints])
        assert np.abs(got[..., 1:3] - want[..., 1:3]).max() <= 2 ** -8  # one bf16 ulp below 1 on a 1e-5 difference
        rot, ph = pol.act(env.obs, env.agent_state, logits=logits, env=env)
        ref = bf16_logits(pol, env.obs.to(torch.float32), env.agent_state)
        assert torch.allclose(logits, ref, rtol=0, atol=3e-3), float((logits - ref).abs().max())
        rot_h, ph_h = rot.cpu().numpy(), ph.cpu().numpy()
        assert set(np.unique(rot_h)) <= {-1, 0, 1} and set(np.unique(ph_h)) <= {0, 1, 2}
        jit = rng.random((E, N))
        obs, ast, rew, done = env.step_update(rot, ph, jit)
        o_obs, o_ast, o_rew, o_done = orc.step(rot_h[pick], ph_h[pick])
        orc.update(jit[pick])
        np.testing.assert_array_equal(rew[pick].cpu().numpy(), o_rew.astype(np.float32))
        np.testing.assert_array_equal(ast[pick].cpu().numpy(), o_ast.astype(np.float32))
    xyt = env.read_state(cm.S_ANTS_XYT).cpu().numpy()
    np.testing.assert_allclose(xyt[pick], orc.ants_xyt, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(env.read_state(cm.S_FOOD).cpu().numpy()[pick], orc.food)


@pytest.mark.parametrize("E,N,W,H,R,filt", [
    (8, 512, 256, 256, 8, None),     # c5's shape: 16 full tiles per env, interleaved cell records
    (3, 100, 64, 64, 0, None),       # K = 6, a last tile of 4 ants
    (2, 300, 96, 64, 3, "3x3"),      # explicit sweep mode (separate pheromone / food records), a last tile of 12 ants
    (16, 40, 48, 48, 2, None),       # a small batch: shorter runs per wave (a tile of fewer than 32 ants per workgroup)
    (1, 33, 40, 40, 0, None),
])
def test_inloop_policy_equals_standalone_kernel(E, N, W, H, R, filt):
    """antsrl_set_inloop_policy: the net evaluated inside k_perceive on the rows it has just written must return, bit
    for bit, what antsrl_policy_mlp returns for the stored (bfloat16) observation tensor — in every step, in a
    standalone observation, with and without the pheromone head; and the rows themselves are unchanged by it."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.policy import LinearPolicy
    from antsrl_amd.synth import synth_init
    kw = dict(n_rocks=R, deposit_strength=256.0, act_path=cm.ACT_CELL_META)
    if filt == "3x3":
        f3 = np.ones((3, 3)) * 0.02
        f3[1, 1] = 1 - 8 * 0.02
        kw["filt"] = f3 * 0.999
    cfg = cm.make_cfg(E, N, W, H, **kw)
    init = synth_init(cfg, seed=5, n_food_discs=6, food_rmin=3, food_rmax=6)
    env = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)
    assert env.query(cm.Q_PERCEIVE_RUN) * 4 <= 32, "the in-loop policy needs a 32-ant tile per workgroup"
    plain = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)  # the same run without the in-loop policy
    env.reset(init)
    plain.reset(init)
    F = 49 * cfg.n_channels
    for head in (True, False):
        pol = LinearPolicy(F, env.device, with_pheromone_head=head, seed=7 + head)
        pol.attach(env)
        o, a, _ = env.observe()  # main.py:88: the first observation feeds the first action
        po, pa, _ = plain.observe()
        assert torch.equal(o, po) and torch.equal(a, pa)
        for t in range(5):
            rot_s, ph_s = pol.act(env.obs, env.agent_state, env=env)
            assert torch.equal(env.next_rotation, rot_s), "rotation, step %d" % t
            if head:
                assert torch.equal(env.next_pheromone, ph_s), "pheromone, step %d" % t
            else:
                assert env.next_pheromone is None and ph_s is None
            rot, ph = env.next_rotation.clone(), (env.next_pheromone.clone() if head else None)
            o, a, r, d = env.step_update(rot, ph, None)
            po, pa, pr, pd = plain.step_update(rot, ph, None)
            assert torch.equal(o, po) and torch.equal(a, pa) and torch.equal(r, pr) and torch.equal(d, pd)
        pol.detach(env)
    # detached: observations no longer touch the action buffers
    env.next_rotation.fill_(7)
    env.step_update(None, None, None)
    plain.step_update(None, None, None)
    assert int(env.next_rotation.min()) == 7 and torch.equal(env.obs, plain.obs)


def test_inloop_policy_needs_bfloat16_observations():
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.policy import LinearPolicy
    cfg = cm.make_cfg(2, 64, 64, 64, act_path=cm.ACT_CELL_META)
    env = BatchedAntsEnv(cfg)  # float32 observations
    pol = LinearPolicy(49 * cfg.n_channels, env.device)
    with pytest.raises(AssertionError):
        pol.attach(env)


@pytest.mark.parametrize("K", [6, 7])
def test_policy_kernels_against_the_reference_model_classes(K):
    """(f)2 pinned to the reference: weights, inputs and float32 logits / actions of tests/golden/contract/policy_net_ref.npz
    come from the reference's own `CollectModel(ExploreModel)` (agents/collect_agent.py:24-51, explore_agent_pytorch.py:24-45).
    `LinearPolicy.load_state_dict` takes them; the bf16 MFMA kernel must return the reference's action on every row whose
    float32 top-2 margin exceeds the analytic bf16 error bound, and its logits must lie within that bound of the
    reference's float32 logits."""
    import torch
    from antsrl_amd.policy import LinearPolicy
    from policy_ref import bf16_logit_error_bound, clear_rows, load_policy_fixture
    sd, rec = load_policy_fixture(K)
    dev = torch.device("cuda")
    pol = LinearPolicy(49 * K, dev, seed=0)
    pol.load_state_dict(sd)
    obs = torch.from_numpy(rec["obs"]).to(dev).contiguous()
    ast = torch.from_numpy(rec["agent_state"]).to(dev).contiguous()
    want = torch.from_numpy(np.concatenate([rec["q_rot"], rec["q_ph"]], axis=1)).to(dev)
    logits = torch.empty((obs.shape[0], 6), dtype=torch.float32, device=dev)
    rot, ph = pol.act(obs, ast, logits=logits)
    bound = bf16_logit_error_bound(sd, obs, ast)
    assert bool(((logits - want).abs() <= bound).all()), float(((logits - want).abs() - bound).max())
    n_dis = 0
    for sl, act, ref_act in ((slice(0, 3), rot.long() + 1, rec["a_rot"]), (slice(3, 6), ph.long(), rec["a_ph"])):
        ref_act = torch.from_numpy(ref_act).to(dev)
        clear = clear_rows(want[:, sl], bound[:, sl])
        assert torch.equal(act[clear], ref_act[clear])
        assert float(clear.float().mean()) > 0.5
        n_dis += int((act != ref_act).sum())
    print("K=%d: %d of %d actions differ from the float32 reference net (all inside the bf16 bound)" % (K, n_dis, 2 * obs.shape[0]))


def test_act_only_inloop_policy_full_config5_shard():
    """BASELINE config 5's loop on its full per-GPU shard (512 envs x 512 ants, 256x256), the benched form: the net inside
    k_perceive, (a) writing the bfloat16 observation tensor and (b) act-only (obs == NULL: the rows never leave LDS).
    The actions of (b) equal those of (a) bit for bit in every step, as do reward / agent_state / done.  A third handle
    with float32 observations is driven by the same actions: the reference's float32 net (the fixture's weights, built by
    the reference's CollectModel) on ITS observations gives the disagreement rate of the bf16 in-loop policy — zero on every
    row the bf16 error bound decides; the rate over all rows is written to gpurun_out/c5_policy_disagreement.json."""
    import json
    import os
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.policy import LinearPolicy
    from antsrl_amd.synth import synth_init
    from policy_ref import bf16_logit_error_bound, clear_rows, fp32_logits, load_policy_fixture
    E, N, steps = 512, 512, 6
    cfg = cm.make_cfg(E, N, 256, 256, deposit_strength=256.0)
    init = synth_init(cfg, seed=55)
    sd, _ = load_policy_fixture(6)
    a = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)   # in-loop policy + observation tensor
    b = BatchedAntsEnv(cfg, obs_dtype=torch.bfloat16)   # in-loop policy, act-only
    c = BatchedAntsEnv(cfg)                             # float32 observations: what the reference's net would read
    assert a.query(cm.Q_CELL_META)
    assert a.query(cm.Q_PERCEIVE_RUN) * 4 <= 32, "the in-loop policy needs a 32-ant tile per workgroup"
    pols = []
    for env in (a, b):
        env.reset(init)
        pol = LinearPolicy(49 * cfg.n_channels, env.device, seed=1)
        pol.load_state_dict(sd)
        pol.attach(env)
        pols.append(pol)
    c.reset(init)
    a.observe()
    b.observe(want_obs=False)
    c.observe()
    dis = {"rot": 0, "ph": 0, "rows": 0, "clear_rot": 0, "clear_ph": 0}
    b.obs.fill_(7.0)  # act-only never touches the tensor
    for t in range(steps):
        assert torch.equal(a.next_rotation, b.next_rotation) and torch.equal(a.next_pheromone, b.next_pheromone), "step %d" % t
        # the reference's float32 net on the float32 observation of the same state
        f32 = fp32_logits(sd, c.obs, c.agent_state)
        bound = bf16_logit_error_bound(sd, c.obs, c.agent_state)
        # (the bf16 tensor additionally rounds the pheromone channels: <= 2^-9 relative on inputs the bound already
        #  charges with 2^-9 for the MFMA operand rounding — the in-loop policy rounds ONCE, the same rounding)
        for name, sl, act in (("rot", slice(0, 3), a.next_rotation.reshape(-1).long() + 1), ("ph", slice(3, 6), a.next_pheromone.reshape(-1).long())):
            ref_act = f32[:, sl].argmax(dim=1)
            clear = clear_rows(f32[:, sl], bound[:, sl])
            assert torch.equal(act[clear], ref_act[clear]), "%s, step %d" % (name, t)
            dis[name] += int((act != ref_act).sum())
            dis["clear_" + name] += int(clear.sum())
        dis["rows"] += E * N
        rot, ph = a.next_rotation.clone(), a.next_pheromone.clone()
        oa = a.step_update(rot, ph, None)
        ob = b.step_update(rot, ph, None, want_obs=False)
        c.step_update(rot, ph, None)
        for x, y in zip(oa[1:], ob[1:]):
            assert torch.equal(x, y)
        # the float32 handle saw the same state: same integer channels, rewards, agent_state
        assert torch.equal(oa[2], c.reward) and torch.equal(oa[1], c.agent_state)
        assert torch.equal(oa[0][..., [0, 3, 4, 5]].to(torch.float32), c.obs[..., [0, 3, 4, 5]])
    assert float(b.obs.to(torch.float32).min()) == 7.0 and float(b.obs.to(torch.float32).max()) == 7.0
    dis["rate_rot"] = dis["rot"] / dis["rows"]
    dis["rate_ph"] = dis["ph"] / dis["rows"]
    dis["decided_by_bound_rot"] = dis["clear_rot"] / dis["rows"]
    dis["decided_by_bound_ph"] = dis["clear_ph"] / dis["rows"]
    print("c5 in-loop bf16 policy vs the reference's float32 net:", dis)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        json.dump(dis, open(os.path.join(out, "c5_policy_disagreement.json"), "w"), indent=1)
    assert dis["rate_rot"] < 0.02 and dis["rate_ph"] < 0.02
