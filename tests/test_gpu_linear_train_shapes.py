"""The linear agent's training step (antsrl_lintrain.hip) at the shapes test_gpu_linear_agent.py does not
reach: every k-loop regime of layer1 (F < 16, F % 16 == 0, odd F on 4-byte aligned rows, either side of 64 KiB of LDS, the
widest row), the batch seams (the tile edge, the fused launch against two launches, the grid cap), idx == NULL, rings far
smaller than the batch, the contract's clamps of idx and of the actions, discounts other than 0.5, grads == NULL, and Adam
over 30 steps against torch.optim.Adam.

The reference is contract_train_step in float64 and the bound linear_train_ref.fp32_sum_bounds: a-priori, from the order
of fp32 sums alone, per gradient element and for the loss (test_linear_train_bounds_cpu.py shows it safe and sharp at
these very cases and inputs: linear_train_cases.py).  Ring rows that no index selects are NaN: a stray read shows."""
import ctypes as C

import pytest

import linear_train_cases as K
import linear_train_ref as L
from test_gpu_linear_agent import BOUND_HEADS

pytestmark = pytest.mark.gpu

SENTINEL = 123.0  # what grads holds before a step that must not write it


def _dev(t, misalign):
    """t on the device; misalign: at an address that is 4 and not 8 bytes aligned (a slice [1:] of a larger allocation)."""
    import torch
    if not (misalign and t.dtype == torch.float32):
        return t.cuda().contiguous()
    buf = torch.empty((t.numel() + 1,), dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


def _trainer(case, inp, misalign, **kw):
    import torch
    from antsrl_amd.train import LinearTrainer
    tr = LinearTrainer(case["F"], "cuda", discount=case["discount"], state_dict=inp["sd"], **kw)
    tr.target_l3.copy_(torch.cat([inp["target"][0].reshape(-1), inp["target"][1]]))
    if misalign:
        tr.policy.w1 = _dev(tr.policy.w1.cpu(), True)
    return tr


def _same_bits(a, b, loss_a, loss_b, grads=True):
    import torch
    assert float(loss_a) == float(loss_b)
    assert torch.equal(a.heads, b.heads) and torch.equal(a._adam, b._adam)
    assert not grads or torch.equal(a.grads, b.grads)


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_step_is_inside_the_fp32_sum_bound(case):
    import torch
    F, B, N, discount = case["F"], case["B"], case["N"], case["discount"]
    inp = K.inputs(case)
    misalign = F % 2 == 1
    host_arrays = list(inp["arrays"])
    idx = inp["idx"]
    if idx is not None:  # NaN in every ring row the batch does not hold
        unused = torch.ones((N,), dtype=torch.bool)
        unused[idx] = False
        host_arrays = [a.clone() for a in host_arrays]
        for i in (0, 1, 3, 4, 5):
            host_arrays[i][unused] = float("nan")
    clean = tuple(_dev(a, misalign) for a in host_arrays)           # what the twins train on: clamped already
    arrays, dev_idx = clean, None if idx is None else idx.cuda()
    twin_idx = torch.arange(B, device="cuda") if idx is None else dev_idx
    if case["clamp"] == "idx":
        dev_idx = inp["raw"].cuda()
    elif case["clamp"] == "actions":
        arrays = clean[:2] + (inp["raw"].cuda(),) + clean[3:]
    tr = _trainer(case, inp, misalign)
    ws, launches = C.c_size_t(), C.c_int32()
    assert tr._lib.antsrl_lintrain_sizes(F, B, None, C.byref(ws), C.byref(launches)) == 0
    ntiles = (B + 31) // 32
    blocks = 1 if ntiles <= 16 else min((ntiles + 3) // 4, 1024)
    assert launches.value == (1 if B <= 512 else 2) and ws.value == blocks * 200 * 4
    if B > 131072:
        assert ntiles > 4 * 1024 and ws.value == 1024 * 200 * 4  # the grid is capped: waves loop over tiles

    host = L.new_state(inp["sd"])
    host["target_w3"], host["target_b3"] = inp["target"]
    batch = K.gathered(inp, B)
    loss_ref, g_ref = L.contract_train_step(host, batch, discount, update=False)
    bound = L.fp32_sum_bounds(host, batch, discount)
    before = tr.state_dict()
    tr.grads.fill_(SENTINEL)
    loss = float(tr.step(arrays, dev_idx))
    gd = {k: v.cpu() for k, v in tr.grad_dict().items()}
    err = {k: (gd[k].double() - g_ref[k].double()).abs() for k in L.TRAINED}
    gmax = max(float(g_ref[k].abs().max()) for k in L.TRAINED)
    ratio = L.worst_share(gd, g_ref, bound)
    L.adam(host, gd, tr.lr, tr.betas, tr.eps)
    st, after = tr.adam_state(), tr.state_dict()
    worst_p = max(float((after[k].cpu() - host["sd"][k]).abs().max()) for k in L.TRAINED) / tr.lr
    print("\nMEASURED %s F %d B %d: gradient error %.3g (bound %.3g) of the largest gradient, worst error / bound %.3g; "
          "loss error %.3g (bound %.3g) relative; heads %.3g of a step of lr"
          % (case["name"], F, B, max(float(e.max()) for e in err.values()) / gmax,
             max(float(bound[k].max()) for k in L.TRAINED) / gmax, ratio, abs(loss - loss_ref) / abs(loss_ref),
             bound["loss"] / abs(loss_ref), worst_p))
    for k in L.TRAINED:
        assert bool((err[k] <= bound[k]).all()), (k, float((err[k] / bound[k]).nan_to_num(0.0).max()))
    assert abs(loss - loss_ref) <= bound["loss"]
    # Adam from the device's own gradient: the moments bit for bit, the parameters within BOUND_HEADS of a step
    for k in L.TRAINED:
        assert torch.equal(st["exp_avg"][k].cpu(), host["m"][k]) and torch.equal(st["exp_avg_sq"][k].cpu(), host["v"][k]), k
    assert worst_p <= BOUND_HEADS
    for k in L.NAMES[:2]:
        assert torch.equal(after[k], before[k])
    # grad() then apply() gives the bits of step(): on the clamped batch, on idx = arange(B) where the step had none
    tw = _trainer(case, inp, misalign)
    l2 = tw.grad(clean, twin_idx)
    tw.apply()
    _same_bits(tr, tw, loss, l2)
    # step(keep_grads=False): the same bits everywhere else, grads not written
    tn = _trainer(case, inp, misalign)
    tn.grads.fill_(SENTINEL)
    l3 = tn.step(clean, twin_idx, keep_grads=False)
    _same_bits(tr, tn, loss, l3, grads=False)
    assert bool((tn.grads == SENTINEL).all()) and not bool((tr.grads == SENTINEL).any())


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)])
def test_adam_over_30_steps_against_torch(betas):
    """apply() on supplied gradients, 30 steps, against torch.optim.Adam (foreach=False) on the CPU: the host scalars
    step_size and bc2_sqrt of antsrl_adam_args (antsrl_adam.h) at every step > 1.

    The moments are bit-equal to the restatement of antsrl_adam.h (memory_train_ref.adam_step: every product rounded
    before it is added), as test_adam_stage_matches_torch holds them for the memory agent.  They are NOT bit-equal to
    torch's on the CPU from step 2 on: its vectorised lerp_ fuses a + w * (b - a) into one rounding (26 of 198 elements
    differ in the last bit after one step), so the parameters cannot be derived from equal moments.  The bound is
    therefore the fallback: the worst |restatement - torch| over the same 30 steps on the CPU, times 4.  It is computed
    here, from the CPU alone, and printed."""
    import torch
    from antsrl_amd.train import LinearTrainer
    from memory_train_ref import adam_step
    lr, steps = 1e-3, 30
    tr = LinearTrainer(17, "cuda", lr=lr, betas=betas, seed=6)
    p0 = tr.heads.cpu().clone()
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([param], lr=lr, betas=betas, foreach=False)
    mine = (p0.clone(), torch.zeros(198), torch.zeros(198))
    g = torch.Generator().manual_seed(8)
    kind = torch.randint(0, 5, (198,), generator=g)  # per element: 0 never a gradient, 1 always 1e-12, 2 always 1e3, else random
    cpu_dev = dev_torch = dev_mine = 0.0
    for s in range(1, steps + 1):
        grad = torch.randn((198,), generator=g) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g))
        grad[kind == 0] = 0.0
        grad[kind == 1] = 1e-12
        grad[kind == 2] = 1e3
        if s % 7 == 3:
            grad[kind == 3] = 0.0  # an exact zero between non-zero gradients
        tr.apply(grad.cuda())
        param.grad = grad.clone()
        opt.step()
        mine = adam_step(mine[0], grad, mine[1], mine[2], s, lr, betas[0], betas[1])
        assert torch.equal(tr._adam[0].cpu(), mine[1]) and torch.equal(tr._adam[1].cpu(), mine[2]), s
        got = tr.heads.cpu()
        cpu_dev = max(cpu_dev, float((mine[0] - param.detach()).abs().max()))
        dev_torch = max(dev_torch, float((got - param.detach()).abs().max()))
        dev_mine = max(dev_mine, float((got - mine[0]).abs().max()))
    print("\nMEASURED adam betas %s: 30 steps at lr 1e-3, |device - torch| max %.3g, |device - restatement| max %.3g; "
          "|restatement - torch| on the CPU max %.3g (the bound is 4 x that)" % (betas, dev_torch, dev_mine, cpu_dev))
    assert dev_torch <= 4 * cpu_dev and dev_mine <= 4 * cpu_dev
    assert torch.equal(tr.heads.cpu()[kind == 0], p0[kind == 0])  # never a gradient: never moved
    assert tr.step_count == steps
