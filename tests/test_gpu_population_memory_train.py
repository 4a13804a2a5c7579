"""PopulationMemoryTrainer on the device (antsrl_popmemtrain.hip): member p of a population is, bit for
bit, a MemoryTrainer stepped alone on its slab with its rows, discount and learning rate, whatever P is and whatever
the other members hold; the four shape-compatible exact cases of memory_train_cases equal float64 as one population;
and the host surface.  Every comparison is of bits: there is no tolerance here.

The shapes are the smallest at which the kernels' guards are crossed (memory_train_cases.STAGE's reasons): D = 32 with
a ragged row tile, D = 31, one row, two weight-gradient chunks (B = 257), three loss blocks (B = 513), and the
workload's own."""
import functools
from types import SimpleNamespace

import pytest
import torch

import memory_train_cases as K
from population_harness import RING

pytestmark = pytest.mark.gpu

#: (F, power, mem, B)
SHAPES = [(27, 4, 3, 33), (28, 4, 1, 33), (27, 4, 3, 1), (27, 4, 3, 257), (27, 4, 3, 513), (294, 5, 20, 264)]
SHAPE_IDS = ["F%d-p%d-m%d-B%d" % s for s in SHAPES]
STEPS = 3
FLOATS = ("states", "agent_states", "rewards", "new_states", "new_agent_states")
CANARY = 64  # floats: 256 bytes


def hyper(p):
    """Member p's seed, discount and learning rate: distinct for neighbours."""
    return 11 + p, (0.5, 0.0, 0.99)[p % 3], (1e-4, 1e-3, 1e-5)[p % 3]


def rows_of(B):
    return B + B // 2 + 3


@functools.lru_cache(maxsize=None)
def member_data(shape, p, salt=0):
    """Member p's slab (CPU, the seven arrays in RING's order) and its STEPS index rows with repeats, from a generator
    keyed on the shape, the member and `salt` alone: the same whatever population the member is in."""
    F, power, mem, B = shape
    L = rows_of(B)
    g = torch.Generator().manual_seed(1000003 * salt + 7919 * F + 131 * B + 17 * mem + 1009 * p + 5)
    r = lambda *s: torch.rand(s, generator=g)  # noqa: E731
    slab = ((r(L, F) < 0.3).float() * r(L, F), r(L, 2 + mem) * 2 - 1, torch.randint(0, 3, (L, 2), generator=g),
            torch.randn((L,), generator=g), (r(L, F) < 0.3).float() * r(L, F), r(L, 2 + mem) * 2 - 1, r(L) < 0.3)
    idx = torch.randint(0, L, (STEPS, B), generator=g)
    if B >= 3:
        idx[:, 1], idx[:, 2] = idx[:, 0], idx[:, 0]  # repeats: rows 1 and 2 of a minibatch are row 0 again
    return slab, idx


def make_ring(shape, slabs, nan_unselected=None):
    """A full PopulationReplayMemory of the members' slabs.  nan_unselected = (p, idx): member p's rows that idx does
    not name are NaN in all five float arrays."""
    from antsrl_amd.population import PopulationReplayMemory
    F, _, mem, B = shape
    ring = PopulationReplayMemory(len(slabs), rows_of(B), (F,), device="cuda", agent_states_space=(2 + mem,))
    for p, slab in enumerate(slabs):
        for n, t in zip(RING, slab):
            getattr(ring, n)[p].copy_(t)
    if nan_unselected is not None:
        p, idx = nan_unselected
        dead = torch.ones((rows_of(B),), dtype=torch.bool)
        dead[idx.reshape(-1)] = False
        assert bool(dead.any())
        for n in FLOATS:
            getattr(ring, n)[p][dead.cuda()] = float("nan")
    ring.fill = ring.max_len
    return ring


def make_population(shape, members, **kw):
    from antsrl_amd import population
    F, power, mem, _ = shape
    P = len(members)
    seeds, discount, lr = zip(*[hyper(p) for p in members])
    g = population._Geometry(P, P, 8, 0, F, torch.float32)  # the training entry reads the spec's members and n_features only
    return population.PopulationMemoryTrainer(g, "cuda:0", seeds, discount, lr, update_target_every=1000, power=power,
                                              mem_size=mem, **kw)


def step_population(tr, ring, idxs, loss_into=None):
    """STEPS steps; -> the losses [STEPS, P] and the running loss after each, on the CPU."""
    losses, running = [], []
    for s in range(STEPS):
        idx = torch.stack([i[s] for i in idxs]).cuda().contiguous()
        losses.append(tr.step(ring, idx, loss=loss_into).cpu().clone())
        running.append(tr.running_loss.cpu().clone())
    torch.cuda.synchronize()
    return torch.stack(losses), torch.stack(running)


@functools.lru_cache(maxsize=None)
def alone(shape, p):
    """Member p as a MemoryTrainer of its own, stepped on its slab with its index rows: the reference of every
    comparison, computed once."""
    from antsrl_amd.train import MemoryTrainer
    F, power, mem, _ = shape
    seed, discount, lr = hyper(p)
    slab, idx = member_data(shape, p)
    tr = MemoryTrainer(F, "cuda", discount=discount, lr=lr, power=power, mem_size=mem, seed=seed, update_target_every=1000)
    arrays = tuple(t.cuda().contiguous() for t in slab)
    losses, rl, running = [], None, []
    for s in range(STEPS):
        l = float(tr.step(arrays, idx[s].cuda().contiguous()))
        losses.append(l)
        rl = l if s == 0 else 0.99 * rl + 0.01 * l  # main.py:106-109 in host float64
        running.append(rl)
    return SimpleNamespace(loss=torch.tensor(losses, dtype=torch.float32), running=torch.tensor(running, dtype=torch.float64),
                           grads=tr.grads.cpu().clone(), model=tr._model.cpu().clone(), target=tr._target.cpu().clone(),
                           params_floats=tr.params_floats, trained_floats=tr.trained_floats, sd=tr.state_dict())


def assert_member_is_alone(shape, tr, q, p, losses, running):
    """Member p, at place q of the population `tr`, against its lone run: loss and running loss of every step, the
    gradient of the last, and the whole state block byte for byte (masters, the untrained memory head among them, Adam's
    m and v, both packs), model and target."""
    ref = alone(shape, p)
    assert torch.equal(losses[:, q], ref.loss), ("loss", p, losses[:, q], ref.loss)
    assert torch.equal(running[:, q], ref.running), ("running_loss", p, running[:, q], ref.running)
    assert torch.equal(tr.grads[q].cpu(), ref.grads), ("grads", p)
    assert tr._model[q].numel() == ref.model.numel()
    assert torch.equal(tr._model[q].cpu(), ref.model), ("state block", p)
    assert torch.equal(tr._target[q].cpu(), ref.target), ("target block", p)
    head = slice(ref.trained_floats * 4, ref.params_floats * 4)  # the memory head's masters: never trained
    assert torch.equal(tr._model[q].cpu()[head], tr._target[q].cpu()[head])
    assert tr.adam_state(q)["step"] == STEPS


def run(shape, members):
    tr = make_population(shape, members)
    data = [member_data(shape, p) for p in members]
    losses, running = step_population(tr, make_ring(shape, [d[0] for d in data]), [d[1] for d in data])
    return tr, losses, running


# ---- 1. member p is a MemoryTrainer alone
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_member_is_a_memory_trainer_alone(shape):
    tr, losses, running = run(shape, (0, 1, 2))
    assert len({hyper(p) for p in range(3)}) == 3 and not torch.equal(member_data(shape, 0)[1], member_data(shape, 1)[1])
    for p in range(3):
        assert_member_is_alone(shape, tr, p, p, losses, running)
    assert bool((alone(shape, 0).loss != alone(shape, 1).loss).any())  # the members do differ


# ---- 2. P does not matter
def test_P_does_not_matter():
    shape = SHAPES[0]
    tr1, l1, r1 = run(shape, (0,))
    assert_member_is_alone(shape, tr1, 0, 0, l1, r1)
    from antsrl_amd import _lib
    assert _lib.POP_MAX == 64
    tr64, l64, r64 = run(shape, tuple(range(64)))
    for p in (0, 63):
        assert_member_is_alone(shape, tr64, p, p, l64, r64)
    assert torch.equal(tr64._model[0], tr1._model[0]) and torch.equal(l64[:, 0], l1[:, 0])


# ---- 3. members do not see each other
def _with_canaries(tr, shape):
    """The trainer's grads, workspace and state blocks and a loss tensor moved into allocations that end in 256 bytes of
    canary; -> (the loss tensor, check) where check() asserts every canary intact."""
    P, B = tr.n_members, shape[3]
    canaries = []

    def guarded(t):
        flat = t.reshape(-1)
        fill = 0x5A if t.dtype == torch.uint8 else -7.25
        buf = torch.full((flat.numel() + (256 if t.dtype == torch.uint8 else CANARY),), fill, dtype=t.dtype, device=t.device)
        buf[:flat.numel()].copy_(flat)
        assert buf.data_ptr() % 256 == 0
        canaries.append((buf[flat.numel():], fill))
        return buf[:flat.numel()].view(t.shape)
    tr.grads = guarded(tr.grads)
    tr._model, tr._target = guarded(tr._model), guarded(tr._target)
    tr._work, tr._work_B = guarded(tr.workspace(B)), B
    loss = guarded(torch.zeros((P,), dtype=torch.float32, device="cuda"))

    def check():
        for tail, fill in canaries:
            assert bool((tail == fill).all())
    return loss, check


def test_members_do_not_see_each_other():
    shape = SHAPES[0]
    first, l_first, _ = run(shape, (0, 1, 2))
    # again: members 0 and 2 with other nets (members 40 and 41's seeds and hyper-parameters), slabs and index rows;
    # member 1 as it was, but every row of its slab that its index rows never name is NaN
    tr = make_population(shape, (40, 1, 41))
    loss, check = _with_canaries(tr, shape)
    data = [member_data(shape, 0, salt=1), member_data(shape, 1), member_data(shape, 2, salt=1)]
    ring = make_ring(shape, [d[0] for d in data], nan_unselected=(1, data[1][1]))
    assert bool(torch.isnan(ring.states[1]).any()) and bool(torch.isnan(ring.rewards[1]).any())
    l_second, r_second = step_population(tr, ring, [d[1] for d in data], loss_into=loss)
    check()
    assert torch.equal(l_second[:, 1], l_first[:, 1]) and bool(torch.isfinite(l_second).all())
    assert torch.equal(tr.grads[1], first.grads[1])
    assert torch.equal(tr._model[1], first._model[1]) and torch.equal(tr._target[1], first._target[1])
    assert not torch.equal(tr._model[0], first._model[0]) and not torch.equal(l_second[:, 0], l_first[:, 0])
    assert_member_is_alone(shape, tr, 1, 1, l_second, r_second)


# ---- 4. exact against float64, independent of any device code
EXACT4 = ("F27-p4-m3-B64", "F27-p4-m3-B64-dones-all", "F27-p4-m3-B64-dones-none", "F27-p4-m3-B64-actions")


def test_exact_cases_as_one_population():
    from antsrl_amd import population
    cases = [K.EXACT[K.EXACT_IDS.index(n)] for n in EXACT4]
    inps = [K.exact_inputs(c) for c in cases]
    # the four load into one [4, 64, ...] ring: one shape, one discount, no idx of their own, 64 rows each
    assert len({(K.dims(c), c["B"], c["discount"]) for c in cases}) == 1 and cases[0]["discount"] == 0.5 and cases[0]["B"] == 64
    F, power, mem, n_rot, n_ph = K.dims(cases[0])
    for inp in inps:
        assert inp["idx"] is None and all(t.shape[0] == 64 for t in inp["arrays"])
        assert inp["arrays"][0].shape == (64, F) and inp["arrays"][1].shape == (64, 2 + mem)
    P = 4
    ring = population.PopulationReplayMemory(P, 64, (F,), device="cuda", agent_states_space=(2 + mem,))
    for p, inp in enumerate(inps):
        for n, t in zip(RING, inp["arrays"]):
            getattr(ring, n)[p].copy_(t)
    ring.fill = 64
    g = population._Geometry(P, P, 8, 0, F, torch.float32)
    tr = population.PopulationMemoryTrainer(g, "cuda:0", range(P), [0.5] * P, [2.0 ** -10] * P, betas=(0.5, 0.5),
                                            update_target_every=1000, power=power, mem_size=mem, n_rot=n_rot, n_ph=n_ph)
    for p, inp in enumerate(inps):  # load_state_dict sets both nets: the target's block is taken aside
        tr.load_state_dict(inp["target"], p)
        target = tr._target[p].clone()
        tr.load_state_dict(inp["sd"], p)
        tr._target[p].copy_(target)
    loss = tr.step(ring, torch.arange(64, device="cuda").repeat(P, 1).contiguous()).cpu()
    for p, (c, inp) in enumerate(zip(cases, inps)):
        ref = K.exact_trace(c, inp)
        want = K.flat(ref["grads"])
        got = tr.grads[p].cpu()
        bad = (got.double() != want).nonzero().view(-1)
        assert bad.numel() == 0, (c["name"], bad.numel(), [(int(i), float(got[i]), float(want[i])) for i in bad[:5]])
        assert float(loss[p]) == float(ref["loss"]), (c["name"], float(loss[p]), float(ref["loss"]))
    assert len({float(v) for v in loss}) > 1  # the four are four problems


# ---- 5. the host surface
def test_host_surface():
    from antsrl_amd.population import PopulationReplayMemory
    shape = SHAPES[0]
    F, power, mem, B = shape
    tr, _, _ = run(shape, (0, 1, 2))
    same = lambda a, b: list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)  # noqa: E731
    assert list(tr.state_dict(0)) == list(alone(shape, 0).sd) and len(tr.state_dict(0)) == 26
    # the steps moved the models off their targets; sync_target brings every target back
    assert not any(same(tr.state_dict(p), tr.target_state_dict(p)) for p in range(3))
    tr.sync_target()
    assert tr.syncs == 1 and all(same(tr.state_dict(p), tr.target_state_dict(p)) for p in range(3))
    assert all(torch.equal(tr._target[p][tr._adam_range().stop:], tr._model[p][tr._adam_range().stop:]) for p in range(3))  # the packs
    assert all(tr.adam_state(p)["step"] == tr.step_count == STEPS for p in range(3))
    # load_state_dict(sd, p=1): member 1's model and target, nobody else's, and its Adam moments stay
    before = [tr._model[p].clone() for p in range(3)], [tr._target[p].clone() for p in range(3)]
    moments = tr.adam_state(1)
    assert any(bool((v != 0).any()) for v in moments["exp_avg"].values())
    sd = {k: v.cpu() + 0.125 for k, v in tr.state_dict(1).items()}
    tr.load_state_dict(sd, p=1)
    assert same(tr.state_dict(1), {k: v.cuda() for k, v in sd.items()}) and same(tr.target_state_dict(1), tr.state_dict(1))
    after = tr.adam_state(1)
    assert same(after["exp_avg"], moments["exp_avg"]) and same(after["exp_avg_sq"], moments["exp_avg_sq"])
    for p in (0, 2):
        assert torch.equal(tr._model[p], before[0][p]) and torch.equal(tr._target[p], before[1][p])
    # train(): 0 below min_replay, a [P] device tensor above it
    ring = make_ring(shape, [member_data(shape, p)[0] for p in range(3)])
    assert tr.train(ring, False, minibatch=B, min_replay=len(ring) + 1) == 0 and tr.step_count == STEPS
    loss = tr.train(ring, False, minibatch=B, min_replay=len(ring))
    assert torch.is_tensor(loss) and loss.shape == (3,) and loss.is_cuda and loss.dtype == torch.float32
    assert tr.step_count == STEPS + 1 and tr.last_idx.shape == (3, B) and bool(torch.isfinite(loss).all())
    # a ring built without agent_states_space has exactly the linear populations' shapes
    plain = PopulationReplayMemory(3, 10, (7, 7, 6), device="cuda")
    assert plain.agent_states.shape == (3, 10, 2) == plain.new_agent_states.shape and plain.states.shape == (3, 10, 7, 7, 6)
    assert plain.actions.shape == (3, 10, 2) and plain.rewards.shape == (3, 10) == plain.dones.shape
    wide = PopulationReplayMemory(3, 10, (7, 7, 6), device="cuda", agent_states_space=(2 + mem,))
    assert wide.agent_states.shape == (3, 10, 2 + mem) == wide.new_agent_states.shape
