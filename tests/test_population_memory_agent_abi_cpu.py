"""CPU-side checks of the C-ABI entries of the memory agents' loop for a population (antsrl_pop_memnet_sizes /
antsrl_pop_policy_memory / antsrl_pop_memory_select / antsrl_pop_memory_record_pre / _post; include/antsrl.h, "The
population of memory nets"): exported, the sizes against the single net's, and every invalid argument refused in its own
words before any HIP call.  No kernel is launched here: every call of an enqueueing entry fails validation, and the
pointers are fakes that are never dereferenced (tests/test_population_abi_cpu.py's way).  That an entry ACCEPTS a set of
arguments is shown by the refusal of the LAST thing it checks, a NULL pointer put there on purpose."""
import ctypes as C

import pytest

from abi_fakes import FAKE, ODD, ODD4, ODD128, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib
from population_abi import BF16, FP32, call, shape, spec

NEW = ("antsrl_pop_memnet_sizes", "antsrl_pop_policy_memory", "antsrl_pop_memory_select", "antsrl_pop_memory_record_pre",
       "antsrl_pop_memory_record_post")


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.antsrl_abi_version() == 5  # the entries are additive


POLICY_PTRS = ("packed", "obs", "agent_state", "mem_in", "mem_out", "rotation", "pheromone", "q_out")
SELECT_PTRS = ("rotation", "pheromone", "mem_old", "mem_next", "explored")
PRE_PTRS = ("obs", "agent_state", "memory", "rotation", "pheromone", "states", "agent_states", "actions")
POST_PTRS = ("obs", "agent_state", "memory", "reward", "done", "rewards", "new_states", "new_agent_states", "dones")
RING_ROWS = dict(step=0, K=40, head=0, max_len=200)  # what leads a record entry's arguments
NEXT = C.c_void_p(1 << 24)  # a second fake, far from FAKE: mem_next beside mem_old


def _shape_arg(kw):
    sh = kw.pop("shape", shape())
    return None if sh is None else C.byref(sh)


def policy(lib, s, **kw):
    d = dict({n: FAKE for n in POLICY_PTRS}, shape=_shape_arg(kw), precision=BF16)
    return call(lib.antsrl_pop_policy_memory, s, ("shape", "precision") + POLICY_PTRS, d, kw)


def select(lib, s, **kw):
    d = dict({n: FAKE for n in SELECT_PTRS}, shape=_shape_arg(kw), step=0, mem_next=NEXT)
    return call(lib.antsrl_pop_memory_select, s, ("shape", "step") + SELECT_PTRS, d, kw)


def pre(lib, s, **kw):
    d = dict(RING_ROWS, **{n: FAKE for n in PRE_PTRS}, shape=_shape_arg(kw))
    return call(lib.antsrl_pop_memory_record_pre, s, ("shape",) + tuple(RING_ROWS) + PRE_PTRS, d, kw)


def post(lib, s, **kw):
    d = dict(RING_ROWS, **{n: FAKE for n in POST_PTRS}, shape=_shape_arg(kw))
    return call(lib.antsrl_pop_memory_record_post, s, ("shape",) + tuple(RING_ROWS) + POST_PTRS, d, kw)


def sizes(lib, sh, precision, P):
    stride, total = C.c_size_t(), C.c_size_t()
    rc = lib.antsrl_pop_memnet_sizes(None if sh is None else C.byref(sh), precision, P, C.byref(stride), C.byref(total))
    return rc, stride.value, total.value


ENTRIES = ((policy, b"pop_policy_memory"), (select, b"pop_memory_select"), (pre, b"pop_memory_record_pre"),
           (post, b"pop_memory_record_post"))


# ---- the sizes
@pytest.mark.parametrize("sh", [shape(), shape(F=27, mem=3, power=4), shape(F=1, mem=1, power=4), shape(F=990, mem=32, power=4)])
@pytest.mark.parametrize("P", [1, 3, 64])
def test_sizes_are_the_single_nets_times_P(lib, sh, P):
    one = C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes(C.byref(sh), C.byref(one)) == 0
    rc, stride, total = sizes(lib, sh, BF16, P)
    assert rc == 0 and stride == one.value and total == P * one.value and stride % 256 == 0 and stride > 0
    assert lib.antsrl_pop_memnet_sizes(C.byref(sh), BF16, P, None, None) == 0  # either output may be NULL


@pytest.mark.parametrize("args,code,msg", [
    ((shape(), 2, 3), -1, b"precision 2 is neither"), ((None, 7, 3), -1, b"precision 7 is neither"),
    ((shape(), FP32, 3), -4, b"bf16 operands only"), ((None, BF16, 3), -1, b"NULL shape"),
    ((shape(), BF16, 0), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    ((shape(), BF16, 65), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    ((shape(mem=0), BF16, 3), -1, b"must be >= 1"), ((shape(F=1010), BF16, 3), -4, b"> 1024"),
    ((shape(h1=48), BF16, 3), -4, b"multiples of 32"), ((shape(n_rot=33), BF16, 3), -4, b"n_rot, n_ph"),
    ((shape(mem=33), BF16, 3), -4, b"mem_size 33 > 32")])
def test_sizes_validation(lib, args, code, msg):
    assert sizes(lib, *args)[0] == code, args
    assert msg in lib.antsrl_last_error() and b"pop_memnet_sizes" in lib.antsrl_last_error(), lib.antsrl_last_error()


# ---- the spec and the shape: every enqueueing entry refuses them in the same words, under its own name
@pytest.mark.parametrize("kw,code,msg", [
    (dict(P=0), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    (dict(P=65, E=65), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    (dict(P=3, E=7), -1, b"n_envs = 7 is not a multiple of n_members = 3"),
    (dict(pitch=320), -4, b"dense observation rows: obs_pitch 320 must be 0 or n_features = 294"),
    (dict(E=0), -1, b"n_envs"), (dict(N=0), -1, b"n_ants"), (dict(base=-1), -1, b"env_id_base"),
    (dict(P=1, E=1 << 16, N=1 << 15), -1, b"2^31"),
    (dict(F=0), -1, b"n_features must be >= 1"), (dict(F=1023), -4, b"n_features + 2 = 1025 > 1024"),
    (dict(fmt=2), -1, b"obs_format"),
    (dict(eps=1.5), -1, b"member 0: epsilon must be in [0, 1]"), (dict(eps=float("nan")), -1, b"epsilon must be in [0, 1]"),
    (dict(discount=float("nan")), -1, b"member 0: discount is NaN")])
def test_spec_validation(lib, kw, code, msg):
    for fn, who in ENTRIES:
        assert fn(lib, spec(**kw)) == code, (who, kw)
        err = lib.antsrl_last_error()
        assert msg in err and who in err, (kw, err)


def test_null_spec_and_null_shape(lib):
    for fn, who in ENTRIES:
        assert fn(lib, None) == -1
        assert b"NULL spec" in lib.antsrl_last_error() and who in lib.antsrl_last_error()
        assert fn(lib, spec(), shape=None) == -1
        assert b"NULL shape" in lib.antsrl_last_error() and who in lib.antsrl_last_error()


@pytest.mark.parametrize("sh,code,msg", [
    (shape(mem=0), -1, b"must be >= 1"), (shape(A=0), -1, b"must be >= 1"), (shape(n_ph=0), -1, b"must be >= 1"),
    (shape(A=33), -4, b"agent_dim 33 > 32"), (shape(mem=33), -4, b"mem_size 33 > 32"),
    (shape(h2=96 + 16), -4, b"multiples of 32 and <= 256"), (shape(h3=288), -4, b"multiples of 32 and <= 256"),
    (shape(n_rot=33), -4, b"n_rot, n_ph (33, 3) must be <= 32"), (shape(n_ph=40), -4, b"n_rot, n_ph (3, 40) must be <= 32")])
def test_shape_validation(lib, sh, code, msg):
    for fn, who in ENTRIES:
        assert fn(lib, spec(), shape=sh) == code, (who, msg)
        err = lib.antsrl_last_error()
        assert msg in err and who in err, err


def test_shape_D_limit(lib):
    """F = 1003 passes the spec's own limit (F + 2 <= 1024); with mem_size 20 the net's D is 1025."""
    for fn, who in ENTRIES:
        assert fn(lib, spec(F=1003), shape=shape(F=1003)) == -4
        assert b"= 1025 > 1024" in lib.antsrl_last_error() and who in lib.antsrl_last_error()


def test_features_of_spec_and_shape(lib):
    for fn, who in ENTRIES:
        assert fn(lib, spec(F=294), shape=shape(F=27)) == -1
        err = lib.antsrl_last_error()
        assert b"the spec's n_features = 294 is not the shape's 27" in err and who in err, err


# ---- the acting entry
def test_policy_precision(lib):
    """An unknown precision is refused before any other check (a NULL spec and shape behind it); fp32 is not built."""
    assert policy(lib, None, shape=None, precision=2) == -1
    err = lib.antsrl_last_error()
    assert b"precision 2 is neither ANTSRL_MEMNET_BF16 (0) nor ANTSRL_MEMNET_FP32 (1)" in err and b"pop_policy_memory" in err
    assert policy(lib, spec(), precision=-1) == -1 and b"precision -1 is neither" in lib.antsrl_last_error()
    assert policy(lib, spec(), precision=FP32) == -4
    err = lib.antsrl_last_error()
    assert b"bf16 operands only" in err and b"ANTSRL_MEMNET_FP32" in err and b"pop_policy_memory" in err, err


def test_policy_member_too_large_for_an_int_tile_count(lib):
    """One member of 2^31 - 1 - 100 ants passes the batch rule (below 2^31); rounded up to a workgroup's 128 ants it does
    not fit an int.  2^31 - 1 - 128 ants pass: what is refused next is a pointer."""
    big = (1 << 31) - 1 - 100
    assert policy(lib, spec(P=1, E=1, N=big)) == -4
    err = lib.antsrl_last_error()
    assert b"must fit an int" in err and b"%d" % big in err and b"pop_policy_memory" in err, err
    assert policy(lib, spec(P=1, E=1, N=(1 << 31) - 1 - 128), obs=None) == -1 and b"obs is required" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in POLICY_PTRS if n not in ("pheromone", "q_out")] + [
    (dict(packed=ODD128), b"packed must be 256-byte"), (dict(obs=C.c_void_p((1 << 20) + 1)), b"obs must be 2-byte"),
    (dict(agent_state=ODD), b"agent_state must be 4-byte"), (dict(mem_in=ODD), b"mem_in must be 4-byte"),
    (dict(mem_out=ODD), b"mem_out must be 4-byte"), (dict(q_out=ODD), b"q_out must be 4-byte")])
def test_policy_pointers(lib, kw, msg):
    assert policy(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_policy_memory" in lib.antsrl_last_error(), lib.antsrl_last_error()


def test_policy_f32_obs_alignment(lib):
    assert policy(lib, spec(fmt=0), obs=ODD) == -1 and b"obs must be 4-byte" in lib.antsrl_last_error()


def test_policy_has_no_slice_alignment_rule(lib):
    """Em = 1, n_ants = 33: a member's slice is 19 404 bytes, which the linear populations' acting entries refuse; this
    forward loads element by element and takes it: what is refused next is a pointer."""
    assert policy(lib, spec(P=2, E=2, N=33, fmt=1), rotation=None) == -1 and b"rotation is required" in lib.antsrl_last_error()


# ---- select
@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in SELECT_PTRS if n != "explored"] + [
    (dict(mem_old=ODD), b"mem_old must be 4-byte"), (dict(mem_next=ODD), b"mem_next must be 4-byte")])
def test_select_pointers(lib, kw, msg):
    assert select(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_memory_select" in lib.antsrl_last_error(), lib.antsrl_last_error()


def test_select_overlap(lib):
    """The whole batch's memory is 6 * 20 * 20 * 4 = 9600 bytes: a mem_next that starts inside mem_old's is refused."""
    for off in (4, 9596):
        assert select(lib, spec(), mem_old=FAKE, mem_next=C.c_void_p((1 << 20) + off)) == -1
        assert b"mem_old and mem_next overlap without being equal" in lib.antsrl_last_error()
    assert select(lib, spec(), mem_old=C.c_void_p((1 << 20) + 9596), mem_next=FAKE) == -1
    assert b"overlap" in lib.antsrl_last_error()


# ---- the ring
@pytest.mark.parametrize("kw,msg", [
    (dict(K=41), b"K must be in [1, n_envs / n_members * n_ants = 40] (41)"), (dict(K=0), b"K must be in [1"),
    (dict(max_len=0), b"max_len must be in [1, 2^40]"), (dict(max_len=(1 << 40) + 1), b"max_len must be in [1, 2^40]"),
    (dict(head=-1), b"head must be in [0, max_len = 200)"), (dict(head=200), b"head must be in [0, max_len = 200)")])
def test_record_ring_validation(lib, kw, msg):
    for fn, who in ((pre, b"pop_memory_record_pre"), (post, b"pop_memory_record_post")):
        assert fn(lib, spec(), **kw) == -1, kw
        err = lib.antsrl_last_error()
        assert msg in err and who in err, (kw, err)


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in PRE_PTRS if n != "pheromone"] + [
    (dict(obs=C.c_void_p((1 << 20) + 1)), b"obs must be 2-byte"), (dict(memory=ODD), b"memory must be 4-byte"),
    (dict(states=ODD), b"states must be 4-byte"), (dict(agent_states=ODD), b"agent_states must be 4-byte"),
    (dict(actions=ODD4), b"actions must be 8-byte")])
def test_record_pre_pointers(lib, kw, msg):
    assert pre(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_memory_record_pre" in lib.antsrl_last_error(), lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in POST_PTRS] + [
    (dict(memory=ODD), b"memory must be 4-byte"), (dict(reward=ODD), b"reward must be 4-byte"),
    (dict(new_states=ODD), b"new_states must be 4-byte"), (dict(new_agent_states=ODD), b"new_agent_states must be 4-byte")])
def test_record_post_pointers(lib, kw, msg):
    assert post(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_memory_record_post" in lib.antsrl_last_error(), lib.antsrl_last_error()


# ---- the pair without a memory keeps its arguments and its rules
def test_plain_record_pair_is_as_it_was(lib):
    """antsrl_pop_record_pre / _post take no shape and no memory and accept what they accepted: with the linear
    populations' arguments every check passes up to the last pointer they look at, left NULL here."""
    old_pre = ("obs", "agent_state", "rotation", "pheromone", "states", "agent_states", "actions")
    old_post = ("obs", "agent_state", "reward", "done", "rewards", "new_states", "new_agent_states", "dones")
    for s in (spec(), spec(P=2, E=2, N=33, fmt=0), spec(P=64, E=64, N=1)):
        K = s.n_envs // s.n_members * s.n_ants
        rows = dict(RING_ROWS, K=K)
        d = dict(rows, **dict({n: FAKE for n in old_pre}, actions=None))
        assert call(lib.antsrl_pop_record_pre, s, tuple(rows) + old_pre, d, {}) == -1
        err = lib.antsrl_last_error()
        assert b"pop_record_pre: actions is required" in err, err
        d = dict(rows, **dict({n: FAKE for n in old_post}, dones=None))
        assert call(lib.antsrl_pop_record_post, s, tuple(rows) + old_post, d, {}) == -1
        err = lib.antsrl_last_error()
        assert b"pop_record_post: dones is required" in err, err
    # and a pheromone may still be NULL in the pre half (a net without that head)
    d = dict(RING_ROWS, **dict({n: FAKE for n in old_pre}, pheromone=None, actions=None))
    assert call(lib.antsrl_pop_record_pre, spec(), tuple(RING_ROWS) + old_pre, d, {}) == -1
    assert b"actions is required" in lib.antsrl_last_error()
