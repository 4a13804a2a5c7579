"""CPU-side checks of the memory population's C-ABI entries (antsrl_pop_memtrain_sizes / antsrl_pop_memtrain_step;
include/antsrl.h, "The population of memory nets"): exported, the strides against the single step's sizes and against
memory_train_ref's layouts, and every invalid argument refused in its own words before any HIP call.  No kernel is
launched here: every call of the step fails validation, and the pointers are fakes that are never dereferenced
(tests/test_population_joint_abi_cpu.py's way)."""
import ctypes as C

import pytest

import memory_train_ref as R
from abi_fakes import FAKE, ODD, ODD4, ODD128, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib
from population_abi import call_train, shape, spec

NEW = ("antsrl_pop_memtrain_sizes", "antsrl_pop_memtrain_step")
WHO = b"pop_memtrain_step"


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.antsrl_abi_version() == 5  # the entries are additive


NET_PTRS = ("net_states", "target_states")
RING_PTRS = ("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones")
TRAIN_PTRS = ("shape",) + NET_PTRS + RING_PTRS


def train(lib, s, shp="default", **kw):
    """The step with valid fakes everywhere but in `kw`; shp: an AntsMemNetShape, None (NULL) or the default's."""
    shp = shape() if shp == "default" else shp
    return call_train(lib.antsrl_pop_memtrain_step, s, TRAIN_PTRS, dict(kw, shape=None if shp is None else C.byref(shp)),
                      workspace=FAKE)


def sizes(lib, shp, B, P):
    ss, tf, stride, ws, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = lib.antsrl_pop_memtrain_sizes(None if shp is None else C.byref(shp), B, P, C.byref(ss), C.byref(tf), C.byref(stride),
                                       C.byref(ws), C.byref(n))
    return rc, ss.value, tf.value, stride.value, ws.value, n.value


# ---- the sizes
@pytest.mark.parametrize("F,power,mem", [(27, 4, 3), (28, 4, 1), (294, 5, 20), (990, 5, 32)])
def test_sizes(lib, F, power, mem):
    shp = shape(F, power, mem)
    L = R.state_layout(F, power, mem, 3, 3)
    for B in (1, 33, 264, 513):
        tf1, sb1, ws1 = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.antsrl_memtrain_sizes(C.byref(shp), B, None, C.byref(tf1), C.byref(sb1), C.byref(ws1)) == 0
        W = R.work_layout(F, power, mem, 3, 3, B)
        for P in (1, 3, 64):
            rc, ss, tf, stride, ws, n = sizes(lib, shp, B, P)
            assert rc == 0, lib.antsrl_last_error()
            assert ss == sb1.value == L["bytes"] and ss % 256 == 0, (B, P, ss)
            assert tf == tf1.value == L["trained_floats"]
            assert stride == ws1.value == W["bytes"] and stride % 256 == 0, (B, P, stride)
            assert ws == P * stride and n == 17
    assert lib.antsrl_pop_memtrain_sizes(C.byref(shp), 264, 3, None, None, None, None, None) == 0  # any output may be NULL


@pytest.mark.parametrize("shp,B,P,code,msg", [
    (shape(), 48, 0, -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    (shape(), 48, 65, -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    (shape(), 0, 3, -1, b"B must be >= 1 (0)"), (shape(), (1 << 24) + 1, 3, -4, b"> 16777216 rows"),
    (None, 48, 3, -1, b"NULL shape"), (shape(F=1000, mem=32), 48, 3, -4, b"1034"), (shape(F=0), 48, 3, -1, b"must be >= 1"),
    (shape(mem=33), 48, 3, -4, b"mem_size")])
def test_sizes_validation(lib, shp, B, P, code, msg):
    assert sizes(lib, shp, B, P)[0] == code
    err = lib.antsrl_last_error()
    assert msg in err and b"pop_memtrain_sizes" in err, err


# ---- the spec: refused in the linear population's words, under the entry's own name
@pytest.mark.parametrize("kw,code,msg", [
    (dict(P=0), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    (dict(P=65, E=65), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    (dict(P=3, E=7), -1, b"n_envs = 7 is not a multiple of n_members = 3"),
    (dict(F=0), -1, b"n_features must be >= 1"), (dict(F=1023), -4, b"n_features + 2 = 1025 > 1024"),
    (dict(pitch=320), -4, b"dense observation rows"), (dict(fmt=2), -1, b"obs_format"),
    (dict(eps=1.5), -1, b"member 0: epsilon must be in [0, 1]"), (dict(discount=float("nan")), -1, b"member 0: discount is NaN"),
])
def test_spec_validation(lib, kw, code, msg):
    assert train(lib, spec(**kw)) == code, kw
    err = lib.antsrl_last_error()
    assert msg in err and WHO in err, (kw, err)


def test_null_spec(lib):
    assert train(lib, None) == -1
    assert b"NULL spec" in lib.antsrl_last_error() and WHO in lib.antsrl_last_error()


# ---- the shape
def test_shape(lib):
    assert train(lib, spec(), shp=None) == -1
    assert b"NULL shape" in lib.antsrl_last_error() and WHO in lib.antsrl_last_error()
    # D = 1000 + 2 + 32 = 1034 > 1024, under a spec whose own rule (F + 2 <= 1024) holds
    assert train(lib, spec(F=1000), shp=shape(F=1000, mem=32)) == -4
    err = lib.antsrl_last_error()
    assert b"1034" in err and b"1024" in err and WHO in err, err
    # the spec's rows are not the shape's
    assert train(lib, spec(F=294), shp=shape(F=27, power=4, mem=3)) == -1
    err = lib.antsrl_last_error()
    assert b"the spec's n_features = 294 is not the shape's 27" in err and WHO in err, err


def test_train_B_and_members(lib):
    assert train(lib, spec(), B=0) == -1 and b"B must be >= 1 (0)" in lib.antsrl_last_error() and WHO in lib.antsrl_last_error()
    # 513 rows (three loss blocks) and 64 members pass: the next refusal is a pointer's
    assert train(lib, spec(P=64, E=64), B=513, net_states=None) == -1 and b"net_states is required" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in NET_PTRS + RING_PTRS] + [
    ({n: ODD128}, n.encode() + b" must be 256-byte") for n in NET_PTRS] + [
    ({n: ODD}, n.encode() + b" must be 4-byte") for n in RING_PTRS if n not in ("dones", "actions")] + [
    (dict(actions=ODD4), b"actions must be 8-byte"),
    (dict(idx=None), b"idx is required"), (dict(idx=ODD4), b"idx must be 8-byte"), (dict(loss=None), b"loss is required"),
    (dict(loss=ODD), b"loss must be 4-byte"), (dict(grads=None), b"grads is required"), (dict(grads=ODD), b"grads must be 4-byte"),
    (dict(running_loss=ODD4), b"running_loss must be 8-byte"), (dict(workspace=None), b"workspace is required"),
    (dict(workspace=ODD128), b"workspace must be 256-byte"), (dict(n_rows=0), b"n_rows"),
    (dict(step=0), b"step must be >= 1"), (dict(beta1=1.0), b"beta1, beta2"), (dict(eps=0.0), b"eps must be")])
def test_train_validation(lib, kw, msg):
    assert train(lib, spec(), **kw) == -1, kw
    assert msg in lib.antsrl_last_error() and WHO in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


def test_running_loss_may_be_null_and_member_learning_rate(lib):
    # a NULL running_loss is not what is refused: the next refusal is the step's
    assert train(lib, spec(), running_loss=None, step=0) == -1 and b"step must be >= 1" in lib.antsrl_last_error()
    s = spec()
    s.members[2].learning_rate = -1.0
    assert train(lib, s) == -1 and b"lr must be" in lib.antsrl_last_error() and WHO in lib.antsrl_last_error()
