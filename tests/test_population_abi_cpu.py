"""CPU-side checks of the population's C-ABI entries (antsrl_pop_policy / _select / _record_pre / _record_post /
_lintrain_step; include/antsrl.h, "The population of linear agents"): exported, and every invalid argument refused in
its own words before any HIP call.  No kernel is launched here: every call below fails validation, and the pointers are
fakes that are never dereferenced (tests/test_linear_agent_abi_cpu.py's way)."""
import ctypes as C

import pytest

from abi_fakes import FAKE, ODD, ODD4, ODD8, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib
from population_abi import call, call_train, spec

NEW = ("antsrl_pop_policy", "antsrl_pop_select", "antsrl_pop_record_pre", "antsrl_pop_record_post", "antsrl_pop_lintrain_step")


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.antsrl_abi_version() == 5  # the entries are additive
    assert _lib.POP_MAX == 64
    # the ABI's structs: AntsPopMember {u64 seed, f64 epsilon, f64 learning_rate, f32 discount, i32 reserved} is 32 bytes,
    # AntsPopSpec eight int32 and ANTSRL_POP_MAX = 64 members
    assert C.sizeof(_lib.AntsPopMember) == 32 and C.sizeof(_lib.AntsPopSpec) == 32 + 64 * 32


POLICY_PTRS = ("obs", "agent_state", "w1", "b1", "heads", "target_l3", "rotation", "pheromone")
PRE_PTRS = ("obs", "agent_state", "rotation", "pheromone", "states", "agent_states", "actions")
POST_PTRS = ("obs", "agent_state", "reward", "done", "rewards", "new_states", "new_agent_states", "dones")
TRAIN_PTRS = ("w1", "b1", "heads", "target_l3", "adam", "states", "agent_states", "actions", "rewards", "new_states",
              "new_agent_states", "dones")
RING_ROWS = dict(step=0, K=40, head=0, max_len=200)  # what leads a record entry's arguments


def policy(lib, s, **kw):
    return call(lib.antsrl_pop_policy, s, POLICY_PTRS, {n: FAKE for n in POLICY_PTRS}, kw)


def select(lib, s, **kw):
    return call(lib.antsrl_pop_select, s, ("step", "rotation", "pheromone", "explored"),
                dict(step=0, rotation=FAKE, pheromone=FAKE, explored=None), kw)


def pre(lib, s, **kw):
    return call(lib.antsrl_pop_record_pre, s, tuple(RING_ROWS) + PRE_PTRS, dict(RING_ROWS, **{n: FAKE for n in PRE_PTRS}), kw)


def post(lib, s, **kw):
    return call(lib.antsrl_pop_record_post, s, tuple(RING_ROWS) + POST_PTRS, dict(RING_ROWS, **{n: FAKE for n in POST_PTRS}), kw)


def train(lib, s, **kw):
    return call_train(lib.antsrl_pop_lintrain_step, s, TRAIN_PTRS, kw)


ENTRIES = ((policy, b"pop_policy"), (select, b"pop_select"), (pre, b"pop_record_pre"), (post, b"pop_record_post"),
           (train, b"pop_lintrain_step"))


# ---- the spec: every entry refuses it in the same words, under its own name
SPEC_CASES = [
    (dict(P=0), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    (dict(P=65, E=65), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    (dict(P=3, E=7), -1, b"n_envs = 7 is not a multiple of n_members = 3"),
    (dict(pitch=320), -4, b"dense observation rows: obs_pitch 320 must be 0 or n_features = 294"),
    (dict(E=0), -1, b"n_envs"), (dict(N=0), -1, b"n_ants"), (dict(base=-1), -1, b"env_id_base"),
    (dict(P=1, E=1 << 16, N=1 << 15), -1, b"2^31"),
    (dict(F=0), -1, b"n_features must be >= 1"), (dict(F=1023), -4, b"n_features + 2 = 1025 > 1024"),
    (dict(fmt=2), -1, b"obs_format"),
    (dict(eps=1.5), -1, b"member 0: epsilon must be in [0, 1]"), (dict(eps=float("nan")), -1, b"epsilon must be in [0, 1]"),
    (dict(discount=float("nan")), -1, b"member 0: discount is NaN"),
]


@pytest.mark.parametrize("kw,code,msg", SPEC_CASES)
def test_spec_validation(lib, kw, code, msg):
    for fn, who in ENTRIES:
        assert fn(lib, spec(**kw)) == code, (who, kw)
        err = lib.antsrl_last_error()
        assert msg in err and who in err, (kw, err)


def test_null_spec(lib):
    for fn, who in ENTRIES:
        assert fn(lib, None) == -1
        assert b"NULL spec" in lib.antsrl_last_error() and who in lib.antsrl_last_error()


def test_a_dense_pitch_is_accepted_as_far_as_the_pointers(lib):
    """obs_pitch == n_features is the dense layout under its own name: the refusal that follows is the pointer's."""
    assert policy(lib, spec(pitch=294), obs=None) == -1 and b"obs is required" in lib.antsrl_last_error()


# ---- the acting kernel's alignment rule
def test_policy_alignment_rule(lib):
    """Em = 1, n_ants = 33, F = 294, bfloat16: a member's slice is 19 404 bytes = 16 * 1212 + 12."""
    assert policy(lib, spec(P=2, E=2, N=33, fmt=1)) == -4
    err = lib.antsrl_last_error()
    assert b"pop_policy" in err and b"19404 bytes" in err and b"multiple of 16" in err, err
    # the same ants as float32 rows are 38 808 bytes = 16 * 2425 + 8
    assert policy(lib, spec(P=2, E=2, N=33, fmt=0)) == -4 and b"38808 bytes" in lib.antsrl_last_error()
    # the issue's two test shapes pass the rule (23 520 and 37 632 bytes): what is refused next is a pointer
    for s in (spec(P=3, E=6, N=20, fmt=1), spec(P=2, E=2, N=32, fmt=0)):
        assert policy(lib, s, obs=None) == -1 and b"obs is required" in lib.antsrl_last_error()
    # only the acting kernel has the rule: the other entries take the shape
    assert select(lib, spec(P=2, E=2, N=33), rotation=None) == -1 and b"rotation is required" in lib.antsrl_last_error()
    assert pre(lib, spec(P=2, E=2, N=33), K=33, obs=None) == -1 and b"obs is required" in lib.antsrl_last_error()


def test_policy_flat_form_only(lib):
    """F = 1000: W1 and two 32-row images are 192 KB, more than the LDS: antsrl_policy_mlp falls back, a population does not."""
    assert policy(lib, spec(F=1000)) == -4
    assert b"flat form only" in lib.antsrl_last_error() and b"pop_policy" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in POLICY_PTRS] + [
    (dict(obs=ODD8), b"obs must be 16-byte"), (dict(agent_state=ODD), b"agent_state must be 4-byte"),
    (dict(w1=ODD), b"w1 must be 4-byte"), (dict(heads=ODD), b"heads must be 4-byte"),
    (dict(target_l3=ODD), b"target_l3 must be 4-byte")])
def test_policy_pointers(lib, kw, msg):
    assert policy(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_policy" in lib.antsrl_last_error(), lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [(dict(rotation=None), b"rotation is required"), (dict(pheromone=None), b"pheromone is required")])
def test_select_pointers(lib, kw, msg):
    assert select(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_select" in lib.antsrl_last_error()


# ---- the ring
@pytest.mark.parametrize("kw,msg", [
    (dict(K=41), b"K must be in [1, n_envs / n_members * n_ants = 40] (41)"), (dict(K=0), b"K must be in [1"),
    (dict(max_len=0), b"max_len must be in [1, 2^40]"), (dict(head=-1), b"head must be in [0, max_len = 200)"),
    (dict(head=200), b"head must be in [0, max_len = 200)")])
def test_record_ring_validation(lib, kw, msg):
    for fn, who in ((pre, b"pop_record_pre"), (post, b"pop_record_post")):
        assert fn(lib, spec(), **kw) == -1, kw
        err = lib.antsrl_last_error()
        assert msg in err and who in err, (kw, err)


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in PRE_PTRS if n != "pheromone"] + [
    (dict(obs=C.c_void_p((1 << 20) + 1)), b"obs must be 2-byte"), (dict(states=ODD), b"states must be 4-byte"),
    (dict(actions=ODD4), b"actions must be 8-byte")])
def test_record_pre_pointers(lib, kw, msg):
    assert pre(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_record_pre" in lib.antsrl_last_error(), lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in POST_PTRS] + [
    (dict(reward=ODD), b"reward must be 4-byte"), (dict(new_states=ODD), b"new_states must be 4-byte")])
def test_record_post_pointers(lib, kw, msg):
    assert post(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_record_post" in lib.antsrl_last_error(), lib.antsrl_last_error()


def test_record_f32_obs_alignment(lib):
    assert pre(lib, spec(fmt=0), obs=ODD) == -1 and b"obs must be 4-byte" in lib.antsrl_last_error()


# ---- the training step
def test_train_B(lib):
    assert train(lib, spec(), B=513) == -4
    err = lib.antsrl_last_error()
    assert b"B = 513 > 512 rows" in err and b"pop_lintrain_step" in err, err
    assert train(lib, spec(), B=0) == -1 and b"B must be >= 1" in lib.antsrl_last_error()
    # 512 rows pass: the next refusal is a pointer's
    assert train(lib, spec(), B=512, w1=None) == -1 and b"w1 is required" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in TRAIN_PTRS] + [
    ({n: ODD}, n.encode() + b" must be") for n in TRAIN_PTRS if n != "dones"] + [
    (dict(idx=None), b"idx is required"), (dict(idx=ODD4), b"idx must be 8-byte"), (dict(loss=None), b"loss is required"),
    (dict(loss=ODD), b"loss must be 4-byte"), (dict(grads=ODD), b"grads must be 4-byte"),
    (dict(running_loss=ODD4), b"running_loss must be 8-byte"), (dict(n_rows=0), b"n_rows"),
    (dict(step=0), b"step must be >= 1"), (dict(beta1=1.0), b"beta1, beta2"), (dict(eps=0.0), b"eps must be")])
def test_train_validation(lib, kw, msg):
    assert train(lib, spec(), **kw) == -1, kw
    assert msg in lib.antsrl_last_error() and b"pop_lintrain_step" in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


def test_train_member_learning_rate(lib):
    s = spec()
    s.members[2].learning_rate = -1.0
    assert train(lib, s) == -1 and b"lr must be" in lib.antsrl_last_error()
