"""CPU-side checks of the joint training step's C-ABI entries (antsrl_jointtrain_sizes / _grad / _apply / _step): exported, and
every invalid argument refused with its return code and a message before any HIP call.  No kernel is launched here: every
call below fails validation (or is antsrl_jointtrain_sizes, which is host arithmetic), and the pointers are fakes that are
never dereferenced."""
import ctypes as C

import pytest

import joint_train_ref as J
from antsrl_amd import _lib
from antsrl_amd import build as buildmod

NEW = ("antsrl_jointtrain_sizes", "antsrl_jointtrain_grad", "antsrl_jointtrain_apply", "antsrl_jointtrain_step")
FAKE = C.c_void_p(1 << 20)   # 256-byte aligned
ODD = C.c_void_p((1 << 20) + 2)
ODD4 = C.c_void_p((1 << 20) + 4)
INVALID, UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS


def _blocks(B):
    return ((B + 31) // 32 + 3) // 4


@pytest.mark.parametrize("F", [1, 17, 294, 1022])
@pytest.mark.parametrize("B", [1, 264, 512, 513, 65536])
def test_sizes(lib, F, B):
    tf, ws, n = C.c_size_t(), C.c_size_t(), C.c_int32()
    assert lib.antsrl_jointtrain_sizes(F, B, C.byref(tf), C.byref(ws), C.byref(n)) == 0
    assert tf.value == 32 * (F + 2) + 230
    # the forward stage's partials (200 floats per workgroup of 4 tiles, rounded up to 256 bytes), then dh [B][32]
    assert ws.value == (_blocks(B) * 200 * 4 + 255) // 256 * 256 + B * 32 * 4 == J.work_layout(B)["bytes"]
    assert n.value == 2
    assert lib.antsrl_jointtrain_sizes(F, B, None, None, None) == 0


@pytest.mark.parametrize("F,B,code,msg", [(0, 256, INVALID, b"n_features"), (-3, 256, INVALID, b"n_features"),
                                          (1023, 256, UNSUPPORTED, b"n_features + 2"), (294, 0, INVALID, b"B must be"),
                                          (294, -1, INVALID, b"B must be"), (294, 65537, UNSUPPORTED, b"65536"),
                                          (294, 1 << 40, UNSUPPORTED, b"65536")])
def test_sizes_refusals(lib, F, B, code, msg):
    assert lib.antsrl_jointtrain_sizes(F, B, None, None, None) == code
    err = lib.antsrl_last_error()
    assert msg in err and b"jointtrain_sizes" in err, err


PTRS = ("model", "target_l3", "states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")


def _args(**kw):
    a = dict(F=294, n_rows=1000, idx=FAKE, B=256, discount=0.5, grads=FAKE, loss=FAKE, work=FAKE, m=FAKE, v=FAKE, step=1,
             lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)
    a.update({n: FAKE for n in PTRS})
    a.update(kw)
    return a


def grad(lib, **kw):
    a = _args(**kw)
    return lib.antsrl_jointtrain_grad(a["F"], *[a[n] for n in PTRS], a["n_rows"], a["idx"], a["B"], a["discount"], a["grads"],
                                    a["loss"], a["work"], None)


def step(lib, **kw):
    a = _args(**kw)
    p = [a[n] for n in PTRS]
    return lib.antsrl_jointtrain_step(a["F"], *p[:2], a["m"], a["v"], *p[2:], a["n_rows"], a["idx"], a["B"], a["discount"],
                                    a["step"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["grads"], a["loss"], a["work"], None)


BATCH_CASES = [(dict(F=0), INVALID, b"n_features"), (dict(F=1023), UNSUPPORTED, b"n_features + 2"),
               (dict(B=0), INVALID, b"B must be"), (dict(B=65537), UNSUPPORTED, b"65536"),
               (dict(n_rows=0), INVALID, b"n_rows"), (dict(idx=None, B=256, n_rows=255), INVALID, b"without idx"),
               (dict(idx=ODD4), INVALID, b"idx must be 8-byte"), (dict(grads=ODD), INVALID, b"grads must be 4-byte"),
               (dict(loss=None), INVALID, b"loss is required"), (dict(loss=ODD), INVALID, b"loss must be 4-byte"),
               (dict(work=None), INVALID, b"workspace is required"), (dict(work=ODD4), INVALID, b"workspace must be 256-byte"),
               (dict(discount=float("nan")), INVALID, b"discount is NaN"), (dict(actions=ODD4), INVALID, b"actions must be 8-byte")]
BATCH_CASES += [(dict([(n, None)]), INVALID, n.encode() + b" is required") for n in PTRS]
BATCH_CASES += [(dict([(n, ODD)]), INVALID, n.encode() + b" must be") for n in PTRS if n not in ("dones",)]


@pytest.mark.parametrize("kw,code,msg", BATCH_CASES)
def test_grad_and_step_refusals(lib, kw, code, msg):
    for fn, who in ((grad, b"jointtrain_grad"), (step, b"jointtrain_step")):
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
    assert msg in err and b"jointtrain_step" in err, err


def apply(lib, **kw):
    a = _args(**kw)
    return lib.antsrl_jointtrain_apply(a["F"], a["model"], a["m"], a["v"], a["grads"], a["step"], a["lr"], a["beta1"], a["beta2"],
                                     a["eps"], None)


@pytest.mark.parametrize("kw,code,msg", [(dict(F=0), INVALID, b"n_features"), (dict(F=1023), UNSUPPORTED, b"n_features + 2"),
                                         (dict(model=None), INVALID, b"model is required"), (dict(grads=None), INVALID, b"grads is required"),
                                         (dict(m=ODD), INVALID, b"adam_m must be"), (dict(v=None), INVALID, b"adam_v is required")]
                         + [(kw, INVALID, msg) for kw, msg in ADAM_CASES[:6]])
def test_apply_refusals(lib, kw, code, msg):
    assert apply(lib, **kw) == code
    err = lib.antsrl_last_error()
    assert msg in err and b"jointtrain_apply" in err, err
