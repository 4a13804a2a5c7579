"""CPU-side checks of the rework agent's training entries (antsrl_reworktrain_sizes / _grad / _apply / _step): exported, the
size formulas those of include/antsrl.h, and every invalid argument refused with its return code and a message before any
HIP call.  No kernel is launched here: every call below fails validation (or is antsrl_reworktrain_sizes, which is host
arithmetic), and the pointers are fakes that are never dereferenced."""
import ctypes as C

import pytest
import torch

import rework_train_ref as T
import train_abi as TA
from abi_fakes import INVALID, UNSUPPORTED, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_reworktrain_sizes", "antsrl_reworktrain_grad", "antsrl_reworktrain_apply", "antsrl_reworktrain_step")
FIELDS = [n for n, _ in _lib.AntsReworkShape._fields_]


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


#: the keyword `shape` holds what differs from shape()'s defaults, or None for a NULL shape
KIND = TA.Kind("reworktrain", ("model", "target_collapsed"),
               lambda a: C.byref(shape(**a["shape"])) if a["shape"] is not None else None, ("lead", "model"), dict(shape={}, B=264))
NET_CASES = [(dict(shape=kw), code, msg) for kw, code, msg in SHAPE_CASES]


@pytest.mark.parametrize("kw,code,msg", TA.batch_cases(NET_CASES + [(dict(shape=None), INVALID, b"NULL shape")], KIND))
def test_grad_and_step_refusals(lib, kw, code, msg):
    KIND.check(("grad", "step"), lib, kw, code, msg)


def test_grad_needs_grads_and_step_does_not_say_so(lib):
    KIND.check_grad_needs_grads(lib)


@pytest.mark.parametrize("kw,msg", TA.ADAM_CASES)
def test_step_adam_refusals(lib, kw, msg):
    KIND.check(("step",), lib, kw, INVALID, msg)


@pytest.mark.parametrize("kw,code,msg", TA.apply_cases(NET_CASES))
def test_apply_refusals(lib, kw, code, msg):
    KIND.check(("apply",), lib, kw, code, msg)
