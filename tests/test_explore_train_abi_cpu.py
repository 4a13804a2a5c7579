"""CPU-side checks of the explore agent's C-ABI entries (antsrl_exptrain_sizes / _grad / _apply / _step): exported, and
every invalid argument refused with its return code and a message before any HIP call.  No kernel is launched here: every
call below fails validation (or is antsrl_exptrain_sizes, which is host arithmetic), and the pointers are fakes that are
never dereferenced."""
import ctypes as C

import pytest

import train_abi as TA
from abi_fakes import lib  # noqa: F401 (a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_exptrain_sizes", "antsrl_exptrain_grad", "antsrl_exptrain_apply", "antsrl_exptrain_step")
KIND = TA.Kind("exptrain", ("model", "target"), lambda a: a["F"], ("lead", "model"), dict(F=294, B=256))


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS


def _blocks(B):
    return ((B + 31) // 32 + 3) // 4


@pytest.mark.parametrize("F", [1, 17, 294, 1022])
@pytest.mark.parametrize("B", [1, 256, 512, 513, 65536])
def test_sizes(lib, F, B):
    tf, ws, n = C.c_size_t(), C.c_size_t(), C.c_int32()
    assert lib.antsrl_exptrain_sizes(F, B, C.byref(tf), C.byref(ws), C.byref(n)) == 0
    assert tf.value == 32 * (F + 2) + 32 + 96 + 3
    # the forward stage's partials (104 floats per workgroup of 4 tiles, rounded up to 256 bytes), then dh [B][32]
    assert ws.value == (_blocks(B) * 104 * 4 + 255) // 256 * 256 + B * 32 * 4
    assert n.value == 2
    assert lib.antsrl_exptrain_sizes(F, B, None, None, None) == 0


@pytest.mark.parametrize("F,B,code,msg", TA.SIZES_REFUSALS)
def test_sizes_refusals(lib, F, B, code, msg):
    assert lib.antsrl_exptrain_sizes(F, B, None, None, None) == code
    err = lib.antsrl_last_error()
    assert msg in err and b"exptrain_sizes" in err, err


@pytest.mark.parametrize("kw,code,msg", TA.batch_cases(TA.FEATURE_CASES, KIND))
def test_grad_and_step_refusals(lib, kw, code, msg):
    KIND.check(("grad", "step"), lib, kw, code, msg)


def test_grad_needs_grads_and_step_does_not_say_so(lib):
    KIND.check_grad_needs_grads(lib)


@pytest.mark.parametrize("kw,msg", TA.ADAM_CASES)
def test_step_adam_refusals(lib, kw, msg):
    KIND.check(("step",), lib, kw, TA.INVALID, msg)


@pytest.mark.parametrize("kw,code,msg", TA.apply_cases(TA.FEATURE_CASES))
def test_apply_refusals(lib, kw, code, msg):
    KIND.check(("apply",), lib, kw, code, msg)
