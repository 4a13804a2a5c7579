"""CPU-side checks of the rework agent's training entries (antsrl_reworktrain_sizes / _grad / _apply / _step): exported, the
size formulas those of include/antsrl.h, and every invalid argument refused with its return code and a message before any
HIP call.  No kernel is launched here: every call below fails validation (or is antsrl_reworktrain_sizes, which is host
arithmetic), and the pointers are fakes that are never dereferenced."""
import ctypes as C

import pytest
import torch

import rework_train_ref as T
from antsrl_amd import _lib
from antsrl_amd import build as buildmod

NEW = ("antsrl_reworktrain_sizes", "antsrl_reworktrain_grad", "antsrl_reworktrain_apply", "antsrl_reworktrain_step")
FAKE = C.c_void_p(1 << 20)   # 256-byte aligned
ODD = C.c_void_p((1 << 20) + 2)
ODD4 = C.c_void_p((1 << 20) + 4)
INVALID, UNSUPPORTED = -1, -4
FIELDS = [n for n, _ in _lib.AntsReworkShape._fields_]


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


def shape(**kw):
    v = dict(n_features=294, agent_dim=2, g1=64, g2=128, g3=32, r1=64, r2=128, r3=32, p1=32, n_rot=3, n_ph=3)
    v.update(kw)
    return _lib.AntsReworkShape(*[v[n] for n in FIELDS])


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS


@pytest.mark.parametrize("F,heads,hidden", [(9, (3, 3), None), (62, (2, 5), None), (294, (3, 3), None), (294, (1, 8), T.ODD_HIDDEN),
                                            (1022, (8, 8), None)])
@pytest.mark.parametrize("B", [1, 16, 17, 264, 4096, 4113, 65536])
def test_sizes(lib, F, heads, hidden, B):
    shapes = T.param_shapes(F, *heads, **(hidden or {}))
    sd = {n + ".weight": torch.empty(s) for n, s in shapes.items()}
    sd.update({n + ".bias": torch.empty(s[:1]) for n, s in shapes.items()})
    h = hidden or T.DEFAULT_HIDDEN
    s = shape(n_features=F, n_rot=heads[0], n_ph=heads[1], g1=h["g"][0], g2=h["g"][1], g3=h["g"][2], r1=h["r"][0],
              r2=h["r"][1], r3=h["r"][2], p1=h["p1"])
    pf, ws, n = C.c_size_t(), C.c_size_t(), C.c_int32()
    assert lib.antsrl_reworktrain_sizes(C.byref(s), B, C.byref(pf), C.byref(ws), C.byref(n)) == 0
    assert pf.value == sum(o * i + o for o, i in shapes.values())
    L = T.work_layout(sd, B)
    assert ws.value == L["bytes"]
    assert L["parts"] == min((B + 15) // 16, 256) and L["stride"] % 64 == 0 and L["stride"] >= sum(heads) * (F + 3) + 2
    assert n.value == 4
    assert lib.antsrl_reworktrain_sizes(C.byref(s), B, None, None, None) == 0


SHAPE_CASES = [(dict(n_features=0), INVALID, b"must be >= 1"), (dict(n_rot=0), INVALID, b"must be >= 1"),
               (dict(g2=0), INVALID, b"g2 must be >= 1"), (dict(agent_dim=3), UNSUPPORTED, b"agent_dim 3 is not 2"),
               (dict(n_features=1023), UNSUPPORTED, b"> 1024"), (dict(r1=257), UNSUPPORTED, b"r1 257 > 256"),
               (dict(n_ph=9), UNSUPPORTED, b"must be <= 8")]


@pytest.mark.parametrize("kw,code,msg", SHAPE_CASES)
def test_sizes_shape_refusals(lib, kw, code, msg):
    s = shape(**kw)
    assert lib.antsrl_reworktrain_sizes(C.byref(s), 264, None, None, None) == code
    err = lib.antsrl_last_error()
    assert msg in err and b"reworktrain_sizes" in err, err


@pytest.mark.parametrize("B,code,msg", [(0, INVALID, b"B must be"), (-1, INVALID, b"B must be"), (65537, UNSUPPORTED, b"65536"),
                                        (1 << 40, UNSUPPORTED, b"65536")])
def test_sizes_B_refusals(lib, B, code, msg):
    s = shape()
    assert lib.antsrl_reworktrain_sizes(C.byref(s), B, None, None, None) == code
    err = lib.antsrl_last_error()
    assert msg in err and b"reworktrain_sizes" in err, err
    assert lib.antsrl_reworktrain_sizes(None, 264, None, None, None) == INVALID and b"NULL shape" in lib.antsrl_last_error()


PTRS = ("model", "target_collapsed", "states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")


def _args(**kw):
    a = dict(shape={}, n_rows=1000, idx=FAKE, B=264, discount=0.5, grads=FAKE, loss=FAKE, work=FAKE, m=FAKE, v=FAKE, step=1,
             lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)
    a.update({n: FAKE for n in PTRS})
    a.update(kw)
    a["shape"] = C.byref(shape(**a["shape"])) if a["shape"] is not None else None
    return a


def grad(lib, **kw):
    a = _args(**kw)
    return lib.antsrl_reworktrain_grad(a["shape"], *[a[n] for n in PTRS], a["n_rows"], a["idx"], a["B"], a["discount"],
                                       a["grads"], a["loss"], a["work"], None)


def step(lib, **kw):
    a = _args(**kw)
    p = [a[n] for n in PTRS]
    return lib.antsrl_reworktrain_step(a["shape"], *p[:2], a["m"], a["v"], *p[2:], a["n_rows"], a["idx"], a["B"], a["discount"],
                                       a["step"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["grads"], a["loss"], a["work"], None)


def apply(lib, **kw):
    a = _args(**kw)
    return lib.antsrl_reworktrain_apply(a["shape"], a["model"], a["m"], a["v"], a["grads"], a["step"], a["lr"], a["beta1"],
                                        a["beta2"], a["eps"], None)


BATCH_CASES = [(dict(shape=kw), code, msg) for kw, code, msg in SHAPE_CASES]
BATCH_CASES += [(dict(shape=None), INVALID, b"NULL shape"), (dict(B=0), INVALID, b"B must be"), (dict(B=65537), UNSUPPORTED, b"65536"),
                (dict(n_rows=0), INVALID, b"n_rows"), (dict(idx=None, B=264, n_rows=263), INVALID, b"without idx"),
                (dict(idx=ODD4), INVALID, b"idx must be 8-byte"), (dict(grads=ODD), INVALID, b"grads must be 4-byte"),
                (dict(loss=None), INVALID, b"loss is required"), (dict(loss=ODD), INVALID, b"loss must be 4-byte"),
                (dict(work=None), INVALID, b"workspace is required"), (dict(work=ODD4), INVALID, b"workspace must be 256-byte"),
                (dict(discount=float("nan")), INVALID, b"discount is NaN"), (dict(actions=ODD4), INVALID, b"actions must be 8-byte")]
BATCH_CASES += [(dict([(n, None)]), INVALID, n.encode() + b" is required") for n in PTRS]
BATCH_CASES += [(dict([(n, ODD)]), INVALID, n.encode() + b" must be") for n in PTRS if n not in ("dones",)]


@pytest.mark.parametrize("kw,code,msg", BATCH_CASES)
def test_grad_and_step_refusals(lib, kw, code, msg):
    for fn, who in ((grad, b"reworktrain_grad"), (step, b"reworktrain_step")):
        assert fn(lib, **kw) == code, kw
        err = lib.antsrl_last_error()
        assert msg in err and who in err, (kw, err)


def test_grad_needs_grads_and_step_does_not_say_so(lib):
    assert grad(lib, grads=None) == INVALID and b"grads is required" in lib.antsrl_last_error()
    # (step with grads NULL is valid: checked on the GPU, where it may launch)


ADAM_CASES = [(dict(step=0), b"step must be >= 1"), (dict(lr=-1.0), b"lr"), (dict(lr=float("nan")), b"lr"),
              (dict(beta1=1.0), b"beta1"), (dict(beta2=-0.1), b"beta1, beta2"), (dict(eps=0.0), b"eps"),
              (dict(m=None), b"adam_m is required"), (dict(v=ODD), b"adam_v must be 4-byte")]


@pytest.mark.parametrize("kw,msg", ADAM_CASES)
def test_step_adam_refusals(lib, kw, msg):
    assert step(lib, **kw) == INVALID
    err = lib.antsrl_last_error()
    assert msg in err and b"reworktrain_step" in err, err


@pytest.mark.parametrize("kw,code,msg", [(dict(shape=kw), code, msg) for kw, code, msg in SHAPE_CASES]
                         + [(dict(model=None), INVALID, b"model is required"), (dict(grads=None), INVALID, b"grads is required"),
                            (dict(m=ODD), INVALID, b"adam_m must be"), (dict(v=None), INVALID, b"adam_v is required")]
                         + [(kw, INVALID, msg) for kw, msg in ADAM_CASES[:6]])
def test_apply_refusals(lib, kw, code, msg):
    assert apply(lib, **kw) == code
    err = lib.antsrl_last_error()
    assert msg in err and b"reworktrain_apply" in err, err
