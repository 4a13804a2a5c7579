"""The two populations' kernels stage by stage, off the fused loop's two shapes (antsrl_population.hip, antsrl_popexplore.hip;
DESIGN §7.24 / §7.25, "Held alone at"): k_pop_policy and k_pop_explore_policy, k_pop_select, k_pop_record and k_pop_lintrain
called as entries on synthetic tensors, at the shapes population_stage_cases.py lists and
test_population_stage_cases_cpu.py certifies.

Every stage is held twice: bit for bit to the single agent's entry run member by member on the member's rows, net, seed
and env_id_base + p Em — the populations' defining claim, here at the widths, row counts, member counts, ring phases and
hyper-parameters the loop's shapes do not reach — and to a plain reference that shares no code with either: the net in
float64 on every clear row, the numpy restatement of the draws and the ring, linear_train_ref.contract_train_step under
fp32_sum_bounds.  Every output tensor sits between guard regions of a pattern, asserted untouched.  (The explore
population's training step is held alone by test_gpu_population_explore.py.)"""
import ctypes as C

import numpy as np
import pytest

import linear_train_cases as K
import linear_train_ref as L
import memory_agent_ref as R
import population_stage_cases as S
from agent_harness import ptr, stream
from dqn_ref import RING
from population_harness import COLLECT as H
from population_harness import population_trainer
from test_gpu_linear_agent import BOUND_HEADS

pytestmark = pytest.mark.gpu

PATTERN, GUARD = 0xA5, 256  # the guards' byte, and their size in front of and behind a tensor
SENTINEL = 123.0            # what grads holds before a step


class Guarded:
    """`t`: a tensor of shape and dtype between two guard regions of PATTERN bytes (itself PATTERN-filled until written)."""

    def __init__(self, shape, dtype, fill=None):
        import torch
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + n + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.n = n
        assert self.buf.data_ptr() % 256 == 0
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(tuple(shape))
        if fill is not None:
            self.t.fill_(fill)

    def check(self, what=""):
        assert bool((self.buf[:GUARD] == PATTERN).all()), "the guard in front of " + what
        assert bool((self.buf[GUARD + self.n:] == PATTERN).all()), "the guard behind " + what


def _bits(t):
    """A tensor's bits as integers: a NaN fill compares equal to itself."""
    import torch
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _geometry(P, Em, N, base, F, dtype):
    from antsrl_amd.population import _Geometry
    return _Geometry(P, P * Em, N, base, F, dtype)


_henv = []


def _bf16_handle():
    """Only supplies the bfloat16 handle the single policy needs (test_gpu_policy.py's)."""
    import torch
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    if not _henv:
        _henv.append(BatchedAntsEnv(cm.make_cfg(1, 4, 16, 16), obs_dtype=torch.bfloat16))
    return _henv[0]


# ---- acting
@pytest.mark.parametrize("name", S.ACTING_IDS)
@pytest.mark.parametrize("kind", ["collect", "explore"])
def test_acting(name, kind):
    """Per member: the single LinearPolicy on the member's rows and weights in the same format, bit for bit over all rows;
    the float64 reference's first maximum on every clear row; float32 and bfloat16 observations of the same values give
    equal actions; the explore kernel has no pheromone to write."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.policy import LinearPolicy
    lib = _lib.load()
    c = S.acting_case(name)
    inp, P, Em, N, Mm, F = c["inp"], c["P"], c["Em"], c["N"], c["Mm"], c["F"]
    collect = kind == "collect"
    dev = lambda t: t.cuda().contiguous()  # noqa: E731
    w1, b1, ast = dev(inp["w1"]), dev(inp["b1"]), dev(inp["ast"].reshape(P * Mm, 2))
    heads = dev(torch.cat([inp["w2"].reshape(P, -1), inp["b2"], inp["w3"].reshape(P, -1), inp["b3"]], 1))
    target_l3 = dev(torch.cat([inp["tw3"].reshape(P, -1), inp["tb3"]], 1))
    blocks = dev(S.explore_blocks(inp))
    assert heads.shape == (P, 198) and target_l3.shape == (P, 99) and blocks.shape == (P, 32 * (F + 2) + 131)
    assert not bool((target_l3 == heads[:, 99:]).all(dim=1).any()), "a target layer3 that differs from the live one"
    for p in range(P):
        for q in range(p + 1, P):
            assert not torch.equal(blocks[p], blocks[q]) and not torch.equal(target_l3[p], target_l3[q]), (p, q)
    zeros = [0] * P
    got = {}
    for dtype in (torch.float32, torch.bfloat16):
        obs = dev(inp["obs"].reshape(P * Mm, F)).to(dtype)
        assert torch.equal(obs.float().cpu(), inp["obs"].reshape(P * Mm, F)) and obs.data_ptr() % 16 == 0
        spec = _geometry(P, Em, N, 0, F, dtype).spec(zeros, zeros, [1e-4] * P, zeros)
        rot, ph = Guarded((P * Mm,), torch.int8), Guarded((P * Mm,), torch.int8)
        if collect:
            _lib.check(lib.antsrl_pop_policy(C.byref(spec), ptr(obs), ptr(ast), ptr(w1), ptr(b1), ptr(heads), ptr(target_l3),
                                             ptr(rot.t), ptr(ph.t), stream()), "pop_policy")
        else:
            _lib.check(lib.antsrl_pop_explore_policy(C.byref(spec), ptr(obs), ptr(ast), ptr(blocks), ptr(rot.t), stream()),
                       "pop_explore_policy")
        torch.cuda.synchronize()
        rot.check("rot")
        ph.check("ph")
        if not collect:  # the entry takes no pheromone: the buffer the collect kernel would write kept its pattern
            assert bool((ph.buf == PATTERN).all())
        env = _bf16_handle() if dtype == torch.bfloat16 else None
        for p in range(P):
            rows = slice(p * Mm, (p + 1) * Mm)
            one = LinearPolicy(F, "cuda", with_pheromone_head=collect)
            sd = {"layer1.weight": w1[p], "layer1.bias": b1[p], "layer2.weight": inp["w2"][p], "layer2.bias": inp["b2"][p]}
            if collect:
                sd.update({"layer3.weight": inp["tw3"][p], "layer3.bias": inp["tb3"][p]})
            one.load_state_dict(sd)
            r1, p1 = one.act(obs[rows].view(Mm, 1, 1, F), ast[rows].contiguous(), env=env)
            assert torch.equal(rot.t[rows], r1.reshape(-1)), ("rot against the single policy", p, dtype)
            clear = c["clear"][p].cuda()
            assert torch.equal(rot.t[rows][clear[:, 0]].long().cpu(), c["rot"][p][clear[:, 0].cpu()]), ("rot against float64", p, dtype)
            if collect:
                assert torch.equal(ph.t[rows], p1.reshape(-1)), ("ph against the single policy", p, dtype)
                assert torch.equal(ph.t[rows][clear[:, 1]].long().cpu(), c["ph"][p][clear[:, 1].cpu()]), ("ph against float64", p, dtype)
            else:
                assert p1 is None
        got[dtype] = (rot.t.clone(), ph.t.clone())
    a, b = got[torch.float32], got[torch.bfloat16]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "both observation formats give equal actions"
    assert int(a[0].min()) >= -1 and int(a[0].max()) <= 1 and (not collect or (int(a[1].min()) >= 0 and int(a[1].max()) <= 2))


# ---- select
@pytest.mark.parametrize("name", S.SELECT_IDS)
def test_select(name):
    """antsrl_pop_select against antsrl_agent_select_actions per member (the member's seed, epsilon and env_id_base + p Em)
    and against memory_agent_ref.select; the rows of environments that do not explore keep what the buffers held; once
    more with explored == NULL."""
    import torch
    from antsrl_amd import _lib
    lib = _lib.load()
    c = S.SELECT[name]
    P, Em, N, base, step = c["P"], c["Em"], c["N"], c["base"], c["step"]
    rot0, ph0 = S.select_inputs(c)
    want_r, want_p, want_e = S.select_expected(c, rot0, ph0)
    spec = _geometry(P, Em, N, base, 294, torch.float32).spec(c["seeds"], c["eps"], [1e-4] * P, [0.5] * P)

    def buffers():
        rot, ph = Guarded((P * Em, N), torch.int8), Guarded((P * Em, N), torch.int8)
        rot.t.copy_(torch.from_numpy(rot0))
        ph.t.copy_(torch.from_numpy(ph0))
        return rot, ph
    rot, ph = buffers()
    explored = Guarded((P * Em,), torch.uint8, fill=7)
    _lib.check(lib.antsrl_pop_select(C.byref(spec), step, ptr(rot.t), ptr(ph.t), ptr(explored.t), stream()), "pop_select")
    torch.cuda.synchronize()
    for g, what in ((rot, "rot"), (ph, "ph"), (explored, "explored")):
        g.check(what)
    assert np.array_equal(explored.t.cpu().numpy(), want_e.astype(np.uint8))
    assert np.array_equal(rot.t.cpu().numpy(), want_r) and np.array_equal(ph.t.cpu().numpy(), want_p)
    keep = torch.from_numpy(np.repeat(~want_e, N).reshape(P * Em, N)).cuda()
    assert torch.equal(rot.t[keep].cpu(), torch.from_numpy(rot0)[keep.cpu()]) and torch.equal(ph.t[keep].cpu(), torch.from_numpy(ph0)[keep.cpu()])
    for p in range(P):  # the single agent's entry on the member's rows
        e = slice(p * Em, (p + 1) * Em)
        r1, p1 = torch.from_numpy(rot0[e].copy()).cuda(), torch.from_numpy(ph0[e].copy()).cuda()
        e1 = torch.full((Em,), 7, dtype=torch.uint8, device="cuda")
        _lib.check(lib.antsrl_agent_select_actions(c["seeds"][p], step, base + p * Em, Em, N, c["eps"][p], 3, 3, ptr(r1), ptr(p1),
                                                   ptr(e1), stream()), "agent_select_actions")
        assert torch.equal(rot.t[e], r1) and torch.equal(ph.t[e], p1) and torch.equal(explored.t[e], e1), p
    rot2, ph2 = buffers()
    _lib.check(lib.antsrl_pop_select(C.byref(spec), step, ptr(rot2.t), ptr(ph2.t), None, stream()), "pop_select")  # explored NULL
    torch.cuda.synchronize()
    rot2.check("rot")
    ph2.check("ph")
    assert torch.equal(rot2.t, rot.t) and torch.equal(ph2.t, ph.t)


# ---- record
@pytest.mark.parametrize("name", S.RECORD_IDS)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_record(name, bf16):
    """One step's record_pre and record_post of a PopulationReplayMemory against DeviceReplayMemory's per member
    (env_id_base + p Em, the member's seed) and against the numpy restatement; every ring row not written keeps its NaN
    or sentinel fill; dones come from the right environment of the right member."""
    import torch
    from antsrl_amd.population import PopulationReplayMemory
    from antsrl_amd.replay import DeviceReplayMemory
    c = S.RECORD[name]
    P, Em, N, Lr, space, base, head, step = c["P"], c["Em"], c["N"], c["max_len"], c["space"], c["base"], c["head"], c["step"]
    Mm, F = Em * N, int(np.prod(space))
    k = Mm if c["K"] is None else c["K"]
    inp = S.record_inputs(c)
    want, written = S.record_expected(c, inp)
    dtype = torch.bfloat16 if bf16 else torch.float32
    d = {n: torch.from_numpy(v).cuda() for n, v in inp.items()}
    obs0, obs1 = (d[n].to(dtype).view(P * Mm, *space).contiguous() for n in ("obs0", "obs1"))
    assert torch.equal(obs0.float().view(P * Mm, F), d["obs0"])  # bfloat16 values: both formats record the same floats
    ph = d["ph"] if c["pheromone"] else None
    fills = dict(states=float("nan"), agent_states=float("nan"), actions=S.FILL_ACTION, rewards=float("nan"),
                 new_states=float("nan"), new_agent_states=float("nan"), dones=S.FILL_DONE)

    def filled(ring):
        """The ring's seven arrays replaced by guarded ones holding the fills."""
        guards = {}
        for n in RING:
            t = getattr(ring, n)
            g = Guarded(t.shape, torch.uint8 if t.dtype == torch.bool else t.dtype, fill=fills[n])
            setattr(ring, n, g.t.view(torch.bool) if t.dtype == torch.bool else g.t)
            guards[n] = g
        ring.head = head
        return guards
    ring = PopulationReplayMemory(P, Lr, space, device="cuda")
    guards = filled(ring)
    assert [(ring.states[p].data_ptr() % 16) for p in range(min(P, 3))] == [(p * Lr * F * 4) % 16 for p in range(min(P, 3))]
    spec = _geometry(P, Em, N, base, F, dtype).spec(c["seeds"], [0.0] * P, [1e-4] * P, [0.5] * P)
    ring.record_pre(obs0, d["ast0"], None, d["rot"], ph, spec=spec, step=step, k=k)
    ring.record_post(obs1, d["ast1"], None, d["reward"], d["done"])
    torch.cuda.synchronize()
    for n, g in guards.items():
        g.check(n)
    assert ring.head == R.ring_rows(head, Lr, k)[2]
    for n in RING:  # the numpy restatement, fills included
        got = getattr(ring, n)
        got = got.view(torch.uint8) if got.dtype == torch.bool else got
        assert _same_bits(got.reshape(want[n].shape).cpu(), torch.from_numpy(want[n])), n
    unwritten = torch.from_numpy(~written).cuda()
    assert bool(torch.isnan(ring.states[unwritten]).all()) and bool((ring.dones.view(torch.uint8)[unwritten] == S.FILL_DONE).all())
    for p in range(P):  # the single agent's ring on the member's rows
        rows, envs = slice(p * Mm, (p + 1) * Mm), slice(p * Em, (p + 1) * Em)
        one = DeviceReplayMemory(Lr, space, [2], [2], device="cuda")
        one_guards = filled(one)
        one.record_pre(obs0[rows], d["ast0"][rows], None, d["rot"][rows], None if ph is None else ph[rows], n_envs=Em, n_ants=N,
                       k=c["K"], seed=c["seeds"][p], step=step, env_id_base=base + p * Em)
        one.record_post(obs1[rows], d["ast1"][rows], None, d["reward"][rows], d["done"][envs])
        for n in RING:
            a, b = getattr(ring, n)[p], getattr(one, n)
            assert _same_bits(a.view(torch.uint8) if a.dtype == torch.bool else a, b.view(torch.uint8) if b.dtype == torch.bool else b), (n, p)
            one_guards[n].check(n)
        assert one.head == ring.head


# ---- the collect step alone
@pytest.mark.parametrize("name", S.TRAIN_IDS)
def test_the_collect_step_alone(name):
    """test_gpu_population_explore.py's test_the_step_alone for PopulationLinearTrainer: two consecutive steps; per member
    loss, heads, Adam's moments and grads equal a LinearTrainer of its own on its slab, bit for bit, after each; w1, b1 and
    target_l3 unchanged; the running loss; equal bits for equal inputs.  And the first step against float64: gradient and
    loss inside fp32_sum_bounds per element, the moments bit-equal to Adam from the device's own gradient, the parameters
    within BOUND_HEADS of a step (test_gpu_linear_train_shapes.py's assertions, per member)."""
    import torch
    from antsrl_amd.population import PopulationReplayMemory
    from antsrl_amd.train import LinearTrainer, linear_trained_views
    c = S.train_case(name)
    P, F, B, N = c["P"], c["F"], c["B"], c["N"]
    dev = torch.device("cuda", torch.cuda.current_device())
    inps = [S.train_inputs(c, p) for p in range(P)]
    ring = PopulationReplayMemory(P, N, (F,), device="cuda")
    for i, n in enumerate(RING):
        getattr(ring, n).copy_(torch.stack([inp["ring"][i] for inp in inps]))
    ring.fill = N
    idx = [torch.stack([inp[k] for inp in inps]).cuda() for k in ("idx", "idx2")]
    flat = lambda names, sd: torch.cat([sd[n].reshape(-1) for n in names])  # noqa: E731
    w1 = torch.stack([inp["sd"][K.NAMES[0]] for inp in inps]).cuda()
    b1 = torch.stack([inp["sd"][K.NAMES[1]] for inp in inps]).cuda()
    heads0 = torch.stack([flat(K.NAMES[2:], inp["sd"]) for inp in inps]).cuda()
    target0 = torch.stack([torch.cat([inp["target"][0].reshape(-1), inp["target"][1]]) for inp in inps]).cuda()

    def run():
        tr = population_trainer("PopulationLinearTrainer", P, (F,), dev, c["seeds"], c["discount"], c["lr"])
        g = dict(heads=Guarded((P, 198), torch.float32), adam=Guarded((P, 2, 198), torch.float32, fill=0.0),
                 grads=Guarded((P, 198), torch.float32, fill=SENTINEL), running_loss=Guarded((P,), torch.float64, fill=0.0),
                 loss=Guarded((P,), torch.float32))
        tr.w1.copy_(w1)
        tr.b1.copy_(b1)
        tr.target_l3.copy_(target0)
        g["heads"].t.copy_(heads0)
        tr.heads, tr._adam, tr.grads, tr.running_loss = g["heads"].t, g["adam"].t, g["grads"].t, g["running_loss"].t
        losses = [tr.step(ring, idx[0], loss=g["loss"].t).clone()]
        first = dict(heads=tr.heads.clone(), grads=tr.grads.clone(), adam=tr._adam.clone(), rl=tr.running_loss.clone())
        losses.append(tr.step(ring, idx[1], loss=g["loss"].t).clone())
        torch.cuda.synchronize()
        for n, gd in g.items():
            gd.check(n)
        return tr, losses, first

    tr, losses, first = run()
    assert bool(torch.isfinite(torch.stack(losses)).all()) and not bool((first["grads"] == SENTINEL).any())
    assert torch.equal(tr.w1, w1) and torch.equal(tr.b1, b1) and torch.equal(tr.target_l3, target0), "a step leaves layer1 and the target"
    assert not torch.equal(first["heads"], heads0) and not torch.equal(tr.heads, first["heads"])
    assert torch.equal(first["rl"], losses[0].double()), "the first training step's running loss is its loss"
    # main.py:106-109 in float64, each product rounded before the add (antsrl_monitor.hip's arithmetic)
    assert torch.equal(tr.running_loss, 0.99 * losses[0].double() + 0.01 * losses[1].double())

    worst = dict(g=0.0, gb=0.0, share=0.0, l=0.0, lb=0.0, p=0.0)
    for p in range(P):
        inp = inps[p]
        # ---- a LinearTrainer of its own on its slab
        one = LinearTrainer(F, dev, discount=c["discount"][p], lr=c["lr"][p], update_target_every=1000, state_dict=inp["sd"])
        one.target_l3.copy_(target0[p])
        slab = tuple(getattr(ring, n)[p] for n in RING)
        l0 = one.step(slab, idx[0][p])
        assert torch.equal(l0, losses[0][p]), ("loss", p, 0, float(l0), float(losses[0][p]))
        for what, mine, alone in (("heads", first["heads"][p], one.heads), ("grads", first["grads"][p], one.grads),
                                  ("adam", first["adam"][p], one._adam)):
            assert torch.equal(mine, alone), (what, p, "after the first step")
        l1 = one.step(slab, idx[1][p])  # on the heads and moments the first step moved
        assert torch.equal(l1, losses[1][p]), ("loss", p, 1, float(l1), float(losses[1][p]))
        H.same_trainers(tr, p, one)
        assert tr.step_count == one.step_count == 2
        # ---- the first step against float64
        host = L.new_state(inp["sd"])
        host["target_w3"], host["target_b3"] = inp["target"]
        batch = K.gathered(inp, B)
        loss_ref, g_ref = L.contract_train_step(host, batch, c["discount"][p], update=False)
        bound = L.fp32_sum_bounds(host, batch, c["discount"][p])
        gd = {k: v.cpu() for k, v in linear_trained_views(first["grads"][p]).items()}
        err = {k: (gd[k].double() - g_ref[k].double()).abs() for k in L.TRAINED}
        gmax = max(float(g_ref[k].abs().max()) for k in L.TRAINED)
        loss = float(losses[0][p])
        L.adam(host, gd, c["lr"][p], tr.betas, tr.eps)
        after = linear_trained_views(first["heads"][p])
        worst_p = max(float((after[k].cpu() - host["sd"][k]).abs().max()) for k in L.TRAINED) / c["lr"][p]
        for key, v in (("g", max(float(e.max()) for e in err.values()) / gmax), ("gb", max(float(bound[k].max()) for k in L.TRAINED) / gmax),
                       ("share", L.worst_share(gd, g_ref, bound)), ("l", abs(loss - loss_ref) / abs(loss_ref)),
                       ("lb", bound["loss"] / abs(loss_ref)), ("p", worst_p)):
            worst[key] = max(worst[key], v)
        if p == P - 1:
            print("\nMEASURED %s F %d B %d: gradient error %.3g (bound %.3g) of the largest gradient, worst error / bound %.3g; "
                  "loss error %.3g (bound %.3g) relative; heads %.3g of a step of lr"
                  % (name, F, B, worst["g"], worst["gb"], worst["share"], worst["l"], worst["lb"], worst["p"]))
        for k in L.TRAINED:
            assert bool((err[k] <= bound[k]).all()), (k, p, float((err[k] / bound[k]).nan_to_num(0.0).max()))
        assert abs(loss - loss_ref) <= bound["loss"], p
        m, v = linear_trained_views(first["adam"][p, 0]), linear_trained_views(first["adam"][p, 1])
        for k in L.TRAINED:  # Adam from the device's own gradient: the moments bit for bit
            assert torch.equal(m[k].cpu(), host["m"][k]) and torch.equal(v[k].cpu(), host["v"][k]), (k, p)
        assert worst_p <= BOUND_HEADS, p

    # equal inputs give equal bits
    tr2, losses2, first2 = run()
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    for a, b in ((tr.heads, tr2.heads), (tr.grads, tr2.grads), (tr._adam, tr2._adam), (tr.running_loss, tr2.running_loss),
                 (first["heads"], first2["heads"])):
        assert torch.equal(a, b)
