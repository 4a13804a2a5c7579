"""The stages of the memory agents' loop for a population, each alone: the forward with one pack per
member (antsrl_pop_policy_memory: k_pop_memnet, antsrl_popmemnet.hip), select with the carried memory
(antsrl_pop_memory_select), the ring's record halves with the memory (antsrl_pop_memory_record_pre / _post) and the
trainer's acting packs.  Every comparison is bit for bit against the single entry run on the member's slice with the
member's weights, seed and epsilon; select also against memory_agent_ref's numpy restatement."""
import ctypes as C

import numpy as np
import pytest

import memory_agent_ref as R
from agent_harness import ptr, same_rings, stream
from population_abi import spec as pop_spec
from population_harness import RING, population_trainer

pytestmark = pytest.mark.gpu

CANARY = 0x5A
BF16 = 0  # ANTSRL_MEMNET_BF16


def _guarded(numel, dtype, fill=None):
    """A tensor of `numel` elements with 256 canary bytes behind it: (the tensor, the canary's bytes)."""
    import torch
    esz = torch.empty((), dtype=dtype).element_size()
    raw = torch.full((numel * esz + 256,), CANARY, dtype=torch.uint8, device="cuda")
    t = raw[: numel * esz].view(dtype)
    if fill is not None:
        t.fill_(fill)
    return t, raw[numel * esz:]


def _intact(*canaries):
    return all(bool((c == CANARY).all()) for c in canaries)


class Forward:
    """P members of Mm ants each on (F, power, mem): the nets (a MemoryPolicy per member, distinct seeds), their packs in
    one [P, stride] block and the inputs."""

    def __init__(self, F, power, mem, P, Mm, bf16, seeds=None):
        import torch
        from antsrl_amd import _lib
        from antsrl_amd.policy import MemoryPolicy
        self.lib = _lib.load()
        self.F, self.mem, self.P, self.Mm, self.M = F, mem, P, Mm, P * Mm
        seeds = seeds or [11 + 3 * p for p in range(P)]
        self.pols = [MemoryPolicy(F, "cuda", power=power, mem_size=mem, seed=s) for s in seeds]
        self.shape = self.pols[0].shape
        stride, total = C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.antsrl_pop_memnet_sizes(C.byref(self.shape), BF16, P, C.byref(stride), C.byref(total)))
        assert stride.value == self.pols[0].packed.numel() and total.value == P * stride.value
        self.packs, self.packs_canary = _guarded(total.value, torch.uint8)
        self.packs = self.packs.view(P, stride.value)
        for p, pol in enumerate(self.pols):
            self.packs[p].copy_(pol.packed)
        g = torch.Generator(device="cpu").manual_seed(1000 * F + Mm)
        side = {27: (3, 3, 3), 294: (7, 7, 6)}[F]
        obs = torch.rand((self.M,) + side, generator=g) * 2 - 1
        obs[torch.rand(obs.shape, generator=g) < 0.4] = 0.0
        self.obs = obs.to("cuda", torch.bfloat16 if bf16 else torch.float32).contiguous()
        self.ast = (torch.rand((self.M, 2), generator=g) * 2 - 1).cuda()
        self.mem_in = (torch.rand((self.M, mem), generator=g) * 2 - 1).cuda()
        self.spec = pop_spec(P=P, E=P, N=Mm, F=F, fmt=1 if bf16 else 0)
        self.nq = self.shape.n_rot + self.shape.n_ph

    def outputs(self, with_q=True):
        import torch
        o = {}
        o["mem_out"], o["c_mem"] = _guarded(self.M * self.mem, torch.float32, 7.0)
        o["rot"], o["c_rot"] = _guarded(self.M, torch.int8, 77)
        o["ph"], o["c_ph"] = _guarded(self.M, torch.int8, 77)
        o["q"], o["c_q"] = _guarded(self.M * self.nq, torch.float32, 7.0) if with_q else (None, None)
        return o

    def run(self, o, packs=None, obs=None, ast=None, mem_in=None):
        from antsrl_amd import _lib
        packs, obs = self.packs if packs is None else packs, self.obs if obs is None else obs
        ast, mem_in = self.ast if ast is None else ast, self.mem_in if mem_in is None else mem_in
        _lib.check(self.lib.antsrl_pop_policy_memory(C.byref(self.spec), C.byref(self.shape), BF16, ptr(packs), ptr(obs), ptr(ast),
                                                     ptr(mem_in), ptr(o["mem_out"]), ptr(o["rot"]), ptr(o["ph"]), ptr(o["q"]),
                                                     stream()), "pop_policy_memory")

    def lone(self, p, in_place=False):
        """MemoryPolicy.act of member p's net on its slice -> rot, ph, new memory, q."""
        import torch
        rows = slice(p * self.Mm, (p + 1) * self.Mm)
        q = torch.zeros((self.Mm, self.nq), device="cuda")
        mem = self.mem_in[rows].clone()
        out = None if in_place else torch.zeros_like(mem)
        rot, ph, new = self.pols[p].act(self.obs[rows], self.ast[rows], memory=mem, out=out, q=q)
        return rot.reshape(-1).clone(), ph.reshape(-1).clone(), new.clone(), q

    def same_as_lone(self, o, members, in_place=False):
        import torch
        Mm, mem, nq = self.Mm, self.mem, self.nq
        for p in members:
            rot, ph, new, q = self.lone(p, in_place)
            rows = slice(p * Mm, (p + 1) * Mm)
            assert torch.equal(o["rot"][rows], rot), ("rot", p)
            assert torch.equal(o["ph"][rows], ph), ("ph", p)
            assert torch.equal(o["mem_out"].view(-1, mem)[rows], new), ("memory", p)
            if o["q"] is not None:
                assert torch.equal(o["q"].view(-1, nq)[rows], q), ("q", p)


# Mm: 20 is less than one tile; 40 has a second tile of 8 rows; 136 gives a member two workgroups, the second a single
# partial tile (8 rows) with three spare waves
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("Mm", [20, 40, 136])
@pytest.mark.parametrize("F,power,mem", [(27, 4, 3), (294, 5, 20)])
def test_forward_is_each_members_own(F, power, mem, Mm, bf16):
    import torch
    f = Forward(F, power, mem, 3, Mm, bf16)
    assert not torch.equal(f.packs[0], f.packs[1]) and (Mm + 127) // 128 == (2 if Mm == 136 else 1)
    o = f.outputs()
    f.run(o)
    f.same_as_lone(o, range(3))
    assert _intact(o["c_mem"], o["c_rot"], o["c_ph"], o["c_q"], f.packs_canary)
    # without q_out
    o2 = f.outputs(with_q=False)
    f.run(o2)
    for k in ("rot", "ph", "mem_out"):
        assert torch.equal(o2[k], o[k]), k
    assert _intact(o2["c_mem"], o2["c_rot"], o2["c_ph"])
    # in place: mem_in == mem_out
    o3 = f.outputs()
    o3["mem_out"].copy_(f.mem_in.view(-1))
    f.run(o3, mem_in=o3["mem_out"])
    f.same_as_lone(o3, range(3), in_place=True)
    for k in ("rot", "ph", "mem_out", "q"):
        assert torch.equal(o3[k], o[k]), k
    assert _intact(o3["c_mem"], o3["c_rot"], o3["c_ph"], o3["c_q"])


@pytest.mark.parametrize("P,members", [(1, (0,)), (64, (0, 63))])
def test_forward_at_one_member_and_at_the_most(P, members):
    f = Forward(27, 4, 3, P, 40, False)
    o = f.outputs()
    f.run(o)
    f.same_as_lone(o, members)
    assert _intact(o["c_mem"], o["c_rot"], o["c_ph"], o["c_q"], f.packs_canary)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_forward_reads_and_writes_its_member_only(bf16):
    """Member 1 of three, 40 ants each (a partial last tile beside member 2's first rows).  The other members' packs,
    observations, agent states and memories replaced — by other numbers, then by NaN — leave member 1's outputs as
    they were; under NaN the others' own outputs are NaN, not member 1's; the canaries stay."""
    import torch
    f = Forward(294, 5, 20, 3, 40, bf16)
    Mm, mem, nq = f.Mm, f.mem, f.nq
    mine = slice(Mm, 2 * Mm)
    o = f.outputs()
    f.run(o)
    f.same_as_lone(o, (1,))

    def others(t, value, rows=True):
        """A copy of t with every member's part but member 1's replaced."""
        c = t.clone()
        keep = c[mine].clone() if rows else c[1].clone()
        if value is None:  # other finite numbers: the rows shifted by one, the packs of members 0 and 2 swapped
            c.copy_(torch.flip(t, (0,)) if t.dtype == torch.uint8 else torch.roll(t, 1, 0))
        elif t.dtype == torch.uint8:
            c.fill_(0xFF)  # every bf16 and every fp32 of a pack is a NaN
        else:
            c.fill_(value)
        if rows:
            c[mine] = keep
        else:
            c[1] = keep
        return c

    for value in (None, float("nan")):
        o2 = f.outputs()
        f.run(o2, packs=others(f.packs, value, rows=False), obs=others(f.obs, value), ast=others(f.ast, value),
              mem_in=others(f.mem_in, value))
        assert torch.equal(o2["rot"][mine], o["rot"][mine]) and torch.equal(o2["ph"][mine], o["ph"][mine])
        assert torch.equal(o2["mem_out"].view(-1, mem)[mine], o["mem_out"].view(-1, mem)[mine])
        assert torch.equal(o2["q"].view(-1, nq)[mine], o["q"].view(-1, nq)[mine])
        assert _intact(o2["c_mem"], o2["c_rot"], o2["c_ph"], o2["c_q"])
        if value is not None:
            for p in (0, 2):
                rows = slice(p * Mm, (p + 1) * Mm)
                assert bool(torch.isnan(o2["mem_out"].view(-1, mem)[rows]).all()), ("the memory of member %d is its own NaN" % p)
                assert bool(torch.isnan(o2["q"].view(-1, nq)[rows]).all()), ("q of member %d is its own NaN" % p)
                assert bool((o2["rot"][rows] != 77).all()) and bool((o2["ph"][rows] != 77).all()), "its own workgroups wrote its actions"


# ---- select
@pytest.mark.parametrize("base", [0, 1 << 20])
@pytest.mark.parametrize("N,mem", [(20, 20), (17, 7)], ids=["float4", "float"])
def test_select_with_the_carried_memory(N, mem, base):
    """(17, 7): 17 * 7 floats per environment are no multiple of 4, the float path; (20, 20) the float4 path."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd.policy import memnet_shape
    lib = _lib.load()
    P, Em, F = 3, 2, 27
    eps, seeds = (0.0, 0.5, 1.0), (7, 8, 7)
    assert (N * mem % 4 == 0) == (mem == 20)
    Mm, M = Em * N, P * Em * N
    shape = memnet_shape(F, 4, mem, 3, 3)
    s = pop_spec(P=P, E=P * Em, N=N, F=F, base=base)
    for p in range(P):
        s.members[p].seed, s.members[p].epsilon = seeds[p], eps[p]
    g = torch.Generator(device="cpu").manual_seed(5)
    rot0 = torch.randint(-1, 2, (M,), generator=g).to(torch.int8).cuda()
    ph0 = torch.randint(0, 3, (M,), generator=g).to(torch.int8).cuda()
    old = torch.rand((M, mem), generator=g).cuda()
    new0 = torch.rand((M, mem), generator=g).cuda()
    seen = set()
    for step in (0, 1, 4):  # (member 1's two environments: both explore, neither, and at base 2^20 one of them)
        rot, ph, new = rot0.clone(), ph0.clone(), new0.clone()
        explored = torch.full((P * Em,), 9, dtype=torch.uint8, device="cuda")
        _lib.check(lib.antsrl_pop_memory_select(C.byref(s), C.byref(shape), step, ptr(rot), ptr(ph), ptr(old), ptr(new),
                                                ptr(explored), stream()), "pop_memory_select")
        # explored NULL, and mem_old == mem_next (no memory moves): the same actions
        rot2, ph2, same = rot0.clone(), ph0.clone(), new0.clone()
        _lib.check(lib.antsrl_pop_memory_select(C.byref(s), C.byref(shape), step, ptr(rot2), ptr(ph2), ptr(same), ptr(same),
                                                None, stream()), "pop_memory_select")
        assert torch.equal(rot2, rot) and torch.equal(ph2, ph) and torch.equal(same, new0)
        for p in range(P):
            rows, envs = slice(p * Mm, (p + 1) * Mm), slice(p * Em, (p + 1) * Em)
            r1, p1, n1 = rot0[rows].clone(), ph0[rows].clone(), new0[rows].clone()
            e1 = torch.zeros((Em,), dtype=torch.uint8, device="cuda")
            o1 = old[rows].clone()
            _lib.check(lib.antsrl_agent_select(seeds[p], step, base + p * Em, Em, N, eps[p], 3, 3, mem, ptr(r1), ptr(p1),
                                               ptr(o1), ptr(n1), ptr(e1), stream()), "agent_select")
            assert torch.equal(rot[rows], r1) and torch.equal(ph[rows], p1), ("actions", p, step)
            assert torch.equal(new[rows], n1), ("memory", p, step)
            assert torch.equal(explored[envs], e1), ("explored", p, step)
            # the numpy restatement of the header's text
            wr, wp, wm, wex = R.select(seeds[p], step, base + p * Em, eps[p], 3, 3, rot0[rows].cpu().numpy().reshape(Em, N),
                                       ph0[rows].cpu().numpy().reshape(Em, N), old[rows].cpu().numpy().reshape(Em, N, mem),
                                       new0[rows].cpu().numpy().reshape(Em, N, mem))
            assert np.array_equal(rot[rows].cpu().numpy().reshape(Em, N), wr) and np.array_equal(ph[rows].cpu().numpy().reshape(Em, N), wp)
            assert np.array_equal(new[rows].cpu().numpy().reshape(Em, N, mem), wm)
            assert np.array_equal(explored[envs].cpu().numpy().astype(bool), wex)
            seen.update((p, bool(e)) for e in wex)
    assert {(0, False), (2, True), (1, False), (1, True)} <= seen, "member 1 (epsilon 0.5) explored in some steps and not in others"


# ---- record
def _record_inputs(P, Em, N, bf16, mem, seed):
    import torch
    M = P * Em * N
    g = torch.Generator(device="cpu").manual_seed(seed)
    obs = (torch.rand((M, 7, 7, 6), generator=g) * 2 - 1).to("cuda", torch.bfloat16 if bf16 else torch.float32)
    mk = lambda *shape: torch.rand(shape, generator=g).cuda()  # noqa: E731
    return dict(obs=obs, ast=mk(M, 2), memory=mk(M, mem), rot=torch.randint(-1, 2, (M,), generator=g).to(torch.int8).cuda(),
                ph=torch.randint(0, 3, (M,), generator=g).to(torch.int8).cuda(), obs2=(obs.float() * 0.5 + 0.25).to(obs.dtype),
                ast2=mk(M, 2), memory2=mk(M, mem), reward=mk(M) - 0.5,
                done=(torch.rand((P * Em,), generator=g) < 0.5).to(torch.uint8).cuda())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [None, 24], ids=["all", "stratified"])
@pytest.mark.parametrize("with_memory", [True, False], ids=["memory", "plain"])
def test_record_with_the_carried_memory(with_memory, K, bf16):
    """Three members of 40 ants into a ring of 100 rows from the odd head 77: the call wraps, and rows of 294 floats at an
    odd and at an even row bring up both alignments of the copy.  with_memory False: the (2,) ring through the entries
    that take no memory, as it was."""
    import torch
    from antsrl_amd.policy import memnet_shape
    from antsrl_amd.population import PopulationReplayMemory
    from antsrl_amd.replay import DeviceReplayMemory
    P, Em, N, mem, L, head = 3, 2, 20, 20, 100, 77
    Mm, seeds, step = Em * N, (7, 8, 7), 5
    width = 2 + (mem if with_memory else 0)
    shape = memnet_shape(294, 5, mem, 3, 3)
    s = pop_spec(P=P, E=P * Em, N=N, F=294, fmt=1 if bf16 else 0)
    for p in range(P):
        s.members[p].seed = seeds[p]
    x = _record_inputs(P, Em, N, bf16, mem, seed=21)
    ring = PopulationReplayMemory(P, L, (7, 7, 6), device="cuda", agent_states_space=(width,))
    ring.head = ring.fill = head
    k = Mm if K is None else K
    kw = dict(spec=s, step=step, k=k, **(dict(shape=shape) if with_memory else {}))
    ring.record_pre(x["obs"], x["ast"], x["memory"] if with_memory else None, x["rot"], x["ph"], **kw)
    ring.record_post(x["obs2"], x["ast2"], x["memory2"] if with_memory else None, x["reward"], x["done"])
    assert ring.head == (head + k) % L and ring.fill == L
    assert head + k > L, "the call wraps"
    for p in range(P):
        rows, envs = slice(p * Mm, (p + 1) * Mm), slice(p * Em, (p + 1) * Em)
        one = DeviceReplayMemory(L, (7, 7, 6), [width], [2], device="cuda")
        one.head = one.fill = head
        m1, m2 = (x["memory"][rows], x["memory2"][rows]) if with_memory else (None, None)
        one.record_pre(x["obs"][rows], x["ast"][rows], m1, x["rot"][rows], x["ph"][rows], n_envs=Em, n_ants=N, k=K, seed=seeds[p],
                       step=step, env_id_base=p * Em)
        one.record_post(x["obs2"][rows], x["ast2"][rows], m2, x["reward"][rows], x["done"][envs])
        same_rings(ring.member(p), one, RING)
    if with_memory:
        assert bool((ring.agent_states[:, :, 2:].abs().sum() > 0)), "the memory went into the rows"


def test_a_ring_without_a_memory_still_refuses_one():
    import torch
    from antsrl_amd.population import PopulationReplayMemory
    ring = PopulationReplayMemory(2, 10, (7, 7, 6), device="cuda")
    with pytest.raises(AssertionError, match="no memory"):
        ring.record_pre(None, None, torch.zeros((4, 20), device="cuda"), None, None, spec=None, step=0, k=1)


# ---- the acting packs
def test_packs_are_the_lone_trainers():
    """At construction, after a load and after sync_target, member p's block of `packed` is, byte for byte, the
    MemoryPolicy.packed of a lone MemoryTrainer holding the same state_dict."""
    import torch
    from antsrl_amd.train import MemoryTrainer
    F, seeds = 27, (7, 8, 9)
    tr = population_trainer("PopulationMemoryTrainer", 3, (F,), "cuda", seeds, (0.5, 0.9, 0.99), (1e-3, 1e-4, 1e-3))
    assert tr.packed.shape == (3, tr.pack_stride) and tr.packed.dtype == torch.uint8 and tr.packed.data_ptr() % 256 == 0
    lone = [MemoryTrainer(F, "cuda", seed=s) for s in seeds]
    for p in range(3):
        assert tr.pack_stride == lone[p].policy.packed.numel()
        assert torch.equal(tr.packed[p], lone[p].policy.packed), ("at construction", p)
    assert not torch.equal(tr.packed[0], tr.packed[1])
    # the model moves (as a training step moves it); the acting pack stays the target's until the sync
    before = tr.packed.clone()
    for p in range(3):
        mine, one = tr._views(tr._model[p]), lone[p]._views(lone[p]._model)
        for k in mine:
            mine[k].mul_(1.0 + 0.125 * (p + 1))
            one[k].mul_(1.0 + 0.125 * (p + 1))
    assert torch.equal(tr.packed, before)
    tr.sync_target()
    for p in range(3):
        lone[p].sync_target()
        assert torch.equal(tr.packed[p], lone[p].policy.packed), ("after sync_target", p)
        assert not torch.equal(tr.packed[p], before[p])
    # a load into one member repacks that member and no other
    sd = lone[0].state_dict()
    after_sync = tr.packed.clone()
    tr.load_state_dict(sd, 2)
    lone[2].load_state_dict(sd)
    assert torch.equal(tr.packed[2], lone[2].policy.packed) and torch.equal(tr.packed[2], tr.packed[0])
    assert torch.equal(tr.packed[:2], after_sync[:2])
