"""The workspaces of the linear and the explore trainer, read back (DESIGN §7.11, §7.12 "stage by stage", §7.13): the two
DQN steps that share antsrl_dqn_dev.h, held launch by launch as test_gpu_memory_train_stages.py holds the memory trainer.

a  every [workgroup][output] of the gradient stage's partials lies inside the per-partial bound of linear_train_ref /
   explore_train_ref.partial_bounds (a-priori; test_*_train_bounds_cpu.py show it safe and sharp at these shapes);
b  the finish is an ordered fp32 sum: the gradients and the loss equal the sequential fp32 sum of the device's own
   partials, from 0.0 in workgroup order, bit for bit;
c  the explore step's second stage on its own input: g_w1 and g_b1 against float64 dh^T [bf16 x, bf16 a, 1] on the
   device's own dh, inside gamma(ceil(B / 16) + 16) sum_b |dh| |xe| (one fmaf per row per wave, 15 wave adds), and dh
   against the contract's dq w2[a] inside fp32_sum_bounds' e_dh;
d  nothing is read before it is written and nothing is written outside the layout: the trainer works in a slice of a
   larger buffer between two 4 KiB guards, and a run whose workspace, grads and loss start as zero bytes equals, bit for
   bit, one in which they start as 0xFF bytes (NaN); padding and guards keep their fill;
e  LDS another launch left behind changes nothing: the same grad() before and after a launch at the widest rows and the
   largest grid on all-NaN data gives equal bits, partials included;
f  four fresh trainers in one process on the same arrays at (294, 65536), through step(), grad() + apply(),
   step(keep_grads=False) and grad() + apply(): partials (and dh), gradients, loss, parameters and Adam's state equal the
   first trainer's, one assertion per quantity, and on a difference the message names the workgroups and outputs
   (agent_harness.twin_report).  The linear twins are test_gpu_linear_agent.py::test_step_equals_the_contract's.

d, e and f at linear (294, 65536) compare two launches of k_lintrain at 512 workgroups and so guard its equal bits there
(DESIGN §7.13), as a does at linear_train_cases' inputs, where a workgroup that is off leaves its bound a thousandfold.

Shapes: linear_train_cases.WORKSPACE and explore_train_ref.WORKSPACE_SHAPES, the smallest at which each grid regime
exists.  Ring rows that no index selects are NaN.  -s prints the shares (MEASURED-WORKSPACE lines; recorded in
profiles/dqn_train_workspace.json)."""
import functools
import json
import math

import pytest
import torch

import explore_train_ref as X
import linear_train_cases as K
import linear_train_ref as L
import memory_train_cases as MK
from agent_harness import explore_snapshot, linear_snapshot, random_linear_replay, same_bits, twin_report

pytestmark = pytest.mark.gpu

GUARD = 4096
MODES = ("grad", "step", "step_no_grads")


def _nan_unused(arrays, idx):
    """The ring with NaN in every float of the rows the batch does not hold."""
    unused = torch.ones((arrays[0].shape[0],), dtype=torch.bool)
    unused[idx] = False
    arrays = [a.clone() for a in arrays]
    for i in (0, 1, 3, 4, 5):
        arrays[i][unused] = float("nan")
    return tuple(arrays)


def _share(got, want, bound):
    """The largest |got - want| / bound over the elements (0 / 0 = 0; an error over a zero bound, or a NaN, = inf)."""
    err = (got.double() - want.double()).abs()
    share = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.nan_to_num(share, nan=math.inf).max())


def _fill(t, byte):
    t.view(-1).view(torch.uint8).fill_(byte)
    return t


def _assert_same_bits(first, twin, keys, what):
    """One assertion per quantity; the message is agent_harness.twin_report's localisation, whole."""
    for k in keys:
        if k in twin:
            assert same_bits(first[k], twin[k]), "%s: %s differs%s" % (what, k, twin_report(first, twin))


def _guarded(nbytes, byte):
    """(buffer, offset, the 256-byte aligned slice of nbytes at that offset): GUARD bytes or more on either side, all
    bytes `byte`."""
    buf = torch.full((nbytes + 2 * GUARD + 256,), byte, dtype=torch.uint8, device="cuda")
    off = GUARD + (-(buf.data_ptr() + GUARD)) % 256
    work = buf[off: off + nbytes]
    assert work.data_ptr() % 256 == 0
    return buf, off, work


def _run(tr, mode, arrays, idx, loss=None):
    """One step of `tr` in one of MODES; returns the loss tensor."""
    if mode == "grad":
        loss = tr.grad(arrays, idx, loss=loss)
        tr.apply()
        return loss
    return tr.step(arrays, idx, loss=loss, keep_grads=mode == "step")


# ---- the linear trainer ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lin_host(name):
    """The case, its inputs and its ring with NaN in the unused rows."""
    case = K.WORKSPACE[K.WORKSPACE_IDS.index(name)]
    inp = K.inputs(case)
    return dict(case=case, inp=inp, ring=_nan_unused(inp["arrays"], inp["idx"]))


@functools.lru_cache(maxsize=None)
def _lin_ref(name):
    """(the expected partials, their bound), float64 [workgroups][199]: computed once, never changed."""
    h = _lin_host(name)
    case, inp = h["case"], h["inp"]
    state = L.new_state(inp["sd"])
    state["target_w3"], state["target_b3"] = inp["target"]
    batch = K.gathered(inp, case["B"])
    return L.expected_partials(state, batch, case["discount"]), L.partial_bounds(state, batch, case["discount"])


def _lin_trainer(h):
    from antsrl_amd.train import LinearTrainer
    case, inp = h["case"], h["inp"]
    tr = LinearTrainer(case["F"], "cuda", discount=case["discount"], state_dict=inp["sd"])
    tr.target_l3.copy_(torch.cat([inp["target"][0].reshape(-1), inp["target"][1]]))
    return tr


LIN_INPUTS = ("w1", "b1", "heads_before", "target_l3")


def _lin_step(tr, mode, arrays, idx, B):
    """One step of a LinearTrainer in one of MODES: linear_snapshot, and the net it started from under LIN_INPUTS."""
    before = dict(w1=tr.policy.w1.clone(), b1=tr.policy.b1.clone(), heads_before=tr.heads.clone(), target_l3=tr.target_l3.clone())
    s = linear_snapshot(tr, _run(tr, mode, arrays, idx), B, grads=mode != "step_no_grads")
    s.update({k: v.cpu() for k, v in before.items()})
    return s


def _lin_dev(h):
    return tuple(a.cuda().contiguous() for a in h["ring"]), h["inp"]["idx"].cuda()


@pytest.mark.parametrize("name", K.WORKSPACE_IDS)
def test_linear_partials_inside_their_bound_and_the_finish_is_their_ordered_sum(name):
    h = _lin_host(name)
    B = h["case"]["B"]
    tr = _lin_trainer(h)
    arrays, idx = _lin_dev(h)
    s = linear_snapshot(tr, tr.grad(arrays, idx), B)
    want, bound = _lin_ref(name)
    assert tr._work.numel() == L.work_layout(B)["bytes"] and s["partials"].shape == want.shape
    share = _share(s["partials"], want, bound)
    print("\nMEASURED-WORKSPACE %s" % json.dumps({"case": "linear-" + name, "shares": {"partials": float("%.4g" % share)}}))
    assert share <= 1.0                                                              # a
    total = L.ordered_sum(s["partials"])                                             # b
    assert same_bits(total[:198], s["grads"]), (total[:198] != s["grads"]).nonzero().view(-1).tolist()
    assert same_bits(total[198:], s["loss"]), (float(total[198]), float(s["loss"]))


@pytest.mark.parametrize("name", K.WORKSPACE_IDS)
def test_linear_reads_nothing_before_writing_it_and_writes_inside_the_layout(name):
    h = _lin_host(name)
    B = h["case"]["B"]
    W = L.work_layout(B)
    arrays, idx = _lin_dev(h)
    for mode in MODES:
        runs = []
        for byte in (0x00, 0xFF):
            tr = _lin_trainer(h)
            buf, off, tr._work = _guarded(W["bytes"], byte)
            _fill(tr.grads, byte)
            loss = _run(tr, mode, arrays, idx, loss=_fill(torch.empty((), dtype=torch.float32, device="cuda"), byte))
            assert tr._work.data_ptr() == buf.data_ptr() + off  # the trainer kept the workspace it was handed
            s = linear_snapshot(tr, loss, B, grads=mode != "step_no_grads")
            host = buf.cpu()
            assert bool((host[:off] == byte).all()) and bool((host[off + W["bytes"]:] == byte).all()), (mode, byte, "guards")
            pad = host[off: off + W["bytes"]].view(torch.float32).view(W["blocks"], L.PART)[:, L.OUT:]
            assert bool((pad.contiguous().view(torch.uint8) == byte).all()), (mode, byte, "padding")
            if mode == "step_no_grads":
                assert bool((tr.grads.cpu().view(torch.uint8) == byte).all()), (mode, byte, "grads were to be left alone")
            assert s["finish_ok"], (mode, byte)
            runs.append(s)
        _assert_same_bits(runs[0], runs[1], [k for k in runs[0] if k != "finish_ok"], "%s, zero bytes against 0xFF bytes" % mode)


@functools.lru_cache(maxsize=None)
def _nan_launch_linear():
    """A LinearTrainer at the widest rows with NaN weights, a NaN ring and idx for the largest grid (1024 workgroups, 91 KB
    of LDS each: every CU's LDS is written).  NaN is data here: grad() changes no weight."""
    from antsrl_amd.train import LinearTrainer
    F, B, N = 1022, 131233, 64
    tr = LinearTrainer(F, "cuda")
    for t in (tr.policy.w1, tr.policy.b1, tr.heads, tr.target_l3):
        t.fill_(float("nan"))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    arrays = (nan(N, F), nan(N, 2), torch.zeros((N, 2), dtype=torch.int64, device="cuda"), nan(N), nan(N, F), nan(N, 2),
              torch.zeros((N,), dtype=torch.bool, device="cuda"))
    return tr, arrays, torch.arange(B, device="cuda") % N


@pytest.mark.parametrize("name", K.WORKSPACE_IDS)
def test_linear_is_not_moved_by_the_lds_another_launch_left(name):
    h = _lin_host(name)
    B = h["case"]["B"]
    arrays, idx = _lin_dev(h)
    first = _lin_step(_lin_trainer(h), "grad", arrays, idx, B)
    big, nan_arrays, nan_idx = _nan_launch_linear()
    assert math.isnan(float(big.grad(nan_arrays, nan_idx)))
    again = _lin_step(_lin_trainer(h), "grad", arrays, idx, B)
    _assert_same_bits(first, again, LIN_INPUTS, "the inputs before against after the NaN launch")
    _assert_same_bits(first, again, ("partials", "grads", "loss", "heads", "adam"), "before against after the NaN launch")


@pytest.mark.parametrize("with_done", [False, True])
def test_four_linear_twins_hold_equal_bits(with_done):
    """test_gpu_linear_agent.py::test_step_equals_the_contract's trainers and inputs at (294, 65536), four times over."""
    from antsrl_amd.train import LinearTrainer
    F, N, B = 294, 3000, 65536
    arrays, g = random_linear_replay(N, F, B + with_done, with_done)
    idx = torch.randint(0, N, (B,), device="cuda", generator=g)
    snaps, modes = [], ("step", "grad", "step_no_grads", "grad")
    for mode in modes:
        tr = LinearTrainer(F, "cuda", seed=3 + B % 7)
        tr.target_l3.mul_(0.5)
        snaps.append(_lin_step(tr, mode, arrays, idx, B))
    first = snaps[0]
    assert first["finish_ok"]
    for i, s in enumerate(snaps[1:], 1):
        _assert_same_bits(first, s, LIN_INPUTS, "the inputs of trainer %d (%s)" % (i, modes[i]))
        _assert_same_bits(first, s, ("partials", "grads", "loss", "heads", "adam"), "trainer %d (%s)" % (i, modes[i]))
        assert s["finish_ok"], i


# ---- the explore trainer --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exp_host(F, B):
    """The case and its ring with NaN in the unused rows."""
    state, arrays, idx = X.workspace_case(F, B)
    return dict(F=F, B=B, state=state, arrays=arrays, ring=_nan_unused(arrays, idx), idx=idx)


@functools.lru_cache(maxsize=None)
def _exp_ref(F, B):
    """The expected partials and their bound, the contract's dh and what it may be off by, and xe: computed once."""
    h = _exp_host(F, B)
    state, batch = h["state"], X.gather(h["arrays"], h["idx"])
    f = X.contract_forward(state, batch)
    return dict(want=X.expected_partials(state, batch), bound=X.partial_bounds(state, batch),
                dh=X.contract_backward(state, f)[1], xe=f["xe"], e_dh=X.fp32_sum_bounds(state, batch)["dh"])


def _exp_trainer(h):
    from antsrl_amd.train import ExploreTrainer
    tr = ExploreTrainer(h["F"], "cuda")
    tr.load_state_dict(h["state"]["sd"])
    for k, v in tr._views(tr.target).items():
        v.copy_(h["state"]["target"][k])
    return tr


EXP_INPUTS = ("model_before", "target")


def _exp_step(tr, mode, arrays, idx, B):
    """One step of an ExploreTrainer in one of MODES: explore_snapshot, and the nets it started from under EXP_INPUTS."""
    before = dict(model_before=tr.model.clone(), target=tr.target.clone())
    s = explore_snapshot(tr, _run(tr, mode, arrays, idx), B, grads=mode != "step_no_grads")
    s.update({k: v.cpu() for k, v in before.items()})
    return s


def _exp_dev(h):
    return tuple(a.cuda().contiguous() for a in h["ring"]), h["idx"].cuda()


@pytest.mark.parametrize("F,B", X.WORKSPACE_SHAPES)
def test_explore_stages_inside_their_bounds_and_the_finish_is_an_ordered_sum(F, B):
    h = _exp_host(F, B)
    tr = _exp_trainer(h)
    arrays, idx = _exp_dev(h)
    s = explore_snapshot(tr, tr.grad(arrays, idx), B)
    ref = _exp_ref(F, B)
    assert tr._work.numel() == X.work_layout(B)["bytes"] and s["partials"].shape == ref["want"].shape
    shares = {"partials": _share(s["partials"], ref["want"], ref["bound"])}           # a
    shares["dh"] = _share(s["dh"], ref["dh"], ref["e_dh"])                            # c: dh against the contract's
    xe1 = torch.cat([ref["xe"].double(), torch.ones((B, 1), dtype=torch.float64)], 1)  # c: stage 2 on the device's own dh
    dh = s["dh"].double()
    gd = tr.grad_dict()
    got = torch.cat([gd[X.W1].cpu(), gd[X.B1].cpu()[:, None]], 1)
    shares["layer1"] = _share(got, dh.T @ xe1, X.gamma(-(-B // 16) + 16) * (dh.abs().T @ xe1.abs()))
    print("\nMEASURED-WORKSPACE %s" % json.dumps({"case": "explore-F%d-B%d" % (F, B),
                                                   "shares": {k: float("%.4g" % v) for k, v in shares.items()}}))
    assert max(shares.values()) <= 1.0, shares
    total = X.ordered_sum(s["partials"])                                              # b
    l2 = 32 * (F + 2) + 32
    assert same_bits(total[:99], s["grads"][l2: l2 + 99]), (total[:99] != s["grads"][l2: l2 + 99]).nonzero().view(-1).tolist()
    assert same_bits(total[99:], s["loss"]), (float(total[99]), float(s["loss"]))


@pytest.mark.parametrize("F,B", X.WORKSPACE_SHAPES)
def test_explore_reads_nothing_before_writing_it_and_writes_inside_the_layout(F, B):
    h = _exp_host(F, B)
    W = X.work_layout(B)
    arrays, idx = _exp_dev(h)
    for mode in MODES:
        runs = []
        for byte in (0x00, 0xFF):
            tr = _exp_trainer(h)
            buf, off, tr._work = _guarded(W["bytes"], byte)
            _fill(tr.grads, byte)
            loss = _run(tr, mode, arrays, idx, loss=_fill(torch.empty((), dtype=torch.float32, device="cuda"), byte))
            assert tr._work.data_ptr() == buf.data_ptr() + off
            s = explore_snapshot(tr, loss, B, grads=mode != "step_no_grads")
            host = buf.cpu()
            assert bool((host[:off] == byte).all()) and bool((host[off + W["bytes"]:] == byte).all()), (mode, byte, "guards")
            part = host[off: off + W["blocks"] * X.PART * 4].view(torch.float32).view(W["blocks"], X.PART)[:, X.OUT:]
            gap = host[off + W["blocks"] * X.PART * 4: off + W["dh_offset"]]
            assert bool((part.contiguous().view(torch.uint8) == byte).all()) and bool((gap == byte).all()), (mode, byte, "padding")
            if mode == "step_no_grads":
                assert bool((tr.grads.cpu().view(torch.uint8) == byte).all()), (mode, byte, "grads were to be left alone")
            assert s["finish_ok"], (mode, byte)
            runs.append(s)
        _assert_same_bits(runs[0], runs[1], [k for k in runs[0] if k != "finish_ok"], "%s, zero bytes against 0xFF bytes" % mode)


@functools.lru_cache(maxsize=None)
def _nan_launch_explore():
    """An ExploreTrainer at the widest rows with NaN nets, a NaN ring and idx for the cap of 512 workgroups (151 KB of LDS
    each)."""
    from antsrl_amd.train import ExploreTrainer
    F, B, N = 1022, 65536, 64
    tr = ExploreTrainer(F, "cuda")
    tr.model.fill_(float("nan"))
    tr.target.fill_(float("nan"))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    arrays = (nan(N, F), nan(N, 2), torch.zeros((N, 2), dtype=torch.int64, device="cuda"), nan(N), nan(N, F), nan(N, 2),
              torch.zeros((N,), dtype=torch.bool, device="cuda"))
    return tr, arrays, torch.arange(B, device="cuda") % N


@pytest.mark.parametrize("F,B", X.WORKSPACE_SHAPES)
def test_explore_is_not_moved_by_the_lds_another_launch_left(F, B):
    h = _exp_host(F, B)
    arrays, idx = _exp_dev(h)
    first = _exp_step(_exp_trainer(h), "grad", arrays, idx, B)
    big, nan_arrays, nan_idx = _nan_launch_explore()
    assert math.isnan(float(big.grad(nan_arrays, nan_idx)))
    again = _exp_step(_exp_trainer(h), "grad", arrays, idx, B)
    _assert_same_bits(first, again, EXP_INPUTS, "the inputs before against after the NaN launch")
    _assert_same_bits(first, again, ("partials", "dh", "grads", "loss", "model", "adam"), "before against after the NaN launch")


def test_four_explore_twins_hold_equal_bits():
    F, B = 294, 65536
    h = _exp_host(F, B)
    arrays, idx = _exp_dev(h)
    snaps, modes = [], ("step", "grad", "step_no_grads", "grad")
    for mode in modes:
        tr = _exp_trainer(h)
        snaps.append(_exp_step(tr, mode, arrays, idx, B))
    first = snaps[0]
    assert first["finish_ok"]
    for i, s in enumerate(snaps[1:], 1):
        _assert_same_bits(first, s, EXP_INPUTS, "the inputs of trainer %d (%s)" % (i, modes[i]))
        _assert_same_bits(first, s, ("partials", "dh", "grads", "loss", "model", "adam"), "trainer %d (%s)" % (i, modes[i]))
        assert s["finish_ok"], i


# ---- the memory trainer: read-before-write only (its stages and its padding: test_gpu_memory_train_stages.py) ---------
def test_memory_grad_reads_nothing_before_writing_it():
    import ctypes as C
    from test_gpu_memory_train_stages import _dev, _trainer
    case = MK.STAGE[0]  # the smallest: F = 1, 33 rows
    inp = MK.stage_inputs(case)
    arrays, idx = _dev(inp)
    runs = []
    for byte in (0x00, 0xFF):
        tr = _trainer(case, inp)
        ws = C.c_size_t()
        tr._sizes(case["B"], C.byref(ws), None)
        buf, off, tr._work = _guarded(ws.value, byte)
        _fill(tr.grads, byte)
        loss = tr.grad(arrays, idx, loss=_fill(torch.empty((), dtype=torch.float32, device="cuda"), byte))
        assert tr._work.data_ptr() == buf.data_ptr() + off
        host = buf.cpu()
        assert bool((host[:off] == byte).all()) and bool((host[off + ws.value:] == byte).all()), (byte, "guards")
        runs.append(dict(loss=loss.cpu().reshape(1), grads=tr.grads.cpu()))
    _assert_same_bits(runs[0], runs[1], list(runs[0]), "grad, zero bytes against 0xFF bytes")
