"""CPU-side checks of the joint population's C-ABI entries (antsrl_pop_joint_policy / antsrl_pop_jointtrain_sizes /
antsrl_pop_jointtrain_step; include/antsrl.h, "The population of joint agents"): exported, the sizes against
joint_train_ref's layout restated per member, and every invalid argument refused in its own words before any HIP call.
No kernel is launched here: every call of an enqueueing entry fails validation, and the pointers are fakes that are never
dereferenced (tests/test_population_explore_abi_cpu.py's way).

The contract states no refusal of a workspace STRIDE: the step has antsrl_pop_exptrain_step's argument shape, which
carries none, and computes the stride itself (the launcher behind the entry still refuses one that is short or no
multiple of 256).  What a caller can get wrong is the workspace pointer, refused below; that the stride the entries use
is never short and always a multiple of 256 is test_sizes' and test_stride_over_every_B's."""
import ctypes as C

import pytest

import joint_train_ref as J
from abi_fakes import FAKE, ODD, ODD4, ODD8, ODD128, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib
from population_abi import call, call_train, spec

NEW = ("antsrl_pop_joint_policy", "antsrl_pop_jointtrain_sizes", "antsrl_pop_jointtrain_step")


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.antsrl_abi_version() == 5  # the entries are additive


POLICY_PTRS = ("obs", "agent_state", "model_blocks", "target_l3", "rotation", "pheromone")
TRAIN_PTRS = ("model", "target_l3", "adam_m", "adam_v", "states", "agent_states", "actions", "rewards", "new_states",
              "new_agent_states", "dones")


def policy(lib, s, **kw):
    return call(lib.antsrl_pop_joint_policy, s, POLICY_PTRS, {n: FAKE for n in POLICY_PTRS}, kw)


def train(lib, s, **kw):
    return call_train(lib.antsrl_pop_jointtrain_step, s, TRAIN_PTRS, kw, workspace=FAKE)


def sizes(lib, F, B, P):
    tf, stride, ws, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = lib.antsrl_pop_jointtrain_sizes(F, B, P, C.byref(tf), C.byref(stride), C.byref(ws), C.byref(n))
    return rc, tf.value, stride.value, ws.value, n.value


ENTRIES = ((policy, b"pop_joint_policy"), (train, b"pop_jointtrain_step"))


# ---- the spec: both enqueueing entries refuse it in the linear population's words, under their own names
@pytest.mark.parametrize("kw,code,msg", [
    (dict(P=0), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    (dict(P=65, E=65), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    (dict(P=3, E=7), -1, b"n_envs = 7 is not a multiple of n_members = 3"),
    (dict(F=0), -1, b"n_features must be >= 1"), (dict(F=1023), -4, b"n_features + 2 = 1025 > 1024"),
    (dict(pitch=320), -4, b"dense observation rows"), (dict(fmt=2), -1, b"obs_format"),
    (dict(eps=1.5), -1, b"member 0: epsilon must be in [0, 1]"), (dict(discount=float("nan")), -1, b"member 0: discount is NaN"),
])
def test_spec_validation(lib, kw, code, msg):
    for fn, who in ENTRIES:
        assert fn(lib, spec(**kw)) == code, (who, kw)
        err = lib.antsrl_last_error()
        assert msg in err and who in err, (kw, err)


def test_null_spec(lib):
    for fn, who in ENTRIES:
        assert fn(lib, None) == -1
        assert b"NULL spec" in lib.antsrl_last_error() and who in lib.antsrl_last_error()


# ---- the acting entry
def test_policy_alignment_rule(lib):
    """Em = 1, n_ants = 33, F = 294, bfloat16: a member's slice is 19 404 bytes = 16 * 1212 + 12."""
    assert policy(lib, spec(P=2, E=2, N=33, fmt=1)) == -4
    err = lib.antsrl_last_error()
    assert b"pop_joint_policy" in err and b"19404 bytes" in err and b"multiple of 16" in err, err
    # the acceptance test's two shapes pass the rule: what is refused next is a pointer
    for s in (spec(P=3, E=6, N=20, fmt=1), spec(P=2, E=2, N=32, fmt=0)):
        assert policy(lib, s, obs=None) == -1 and b"obs is required" in lib.antsrl_last_error()


def test_policy_flat_form_only(lib):
    assert policy(lib, spec(F=1000)) == -4
    assert b"flat form only" in lib.antsrl_last_error() and b"pop_joint_policy" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in POLICY_PTRS] + [
    (dict(obs=ODD8), b"obs must be 16-byte"), (dict(agent_state=ODD), b"agent_state must be 4-byte"),
    (dict(model_blocks=ODD), b"model_blocks must be 4-byte"), (dict(target_l3=ODD), b"target_l3 must be 4-byte")])
def test_policy_pointers(lib, kw, msg):
    assert policy(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error() and b"pop_joint_policy" in lib.antsrl_last_error(), lib.antsrl_last_error()


# ---- the sizes
def member_layout(B):
    """joint_train_ref's blocks and work_layout restated per member: the member's part is the single step's, its stride
    that part's bytes rounded up to 256."""
    w = J.work_layout(B)
    assert w["blocks"] == J.blocks(B) and w["dh_offset"] % 256 == 0 and w["dh_offset"] >= J.blocks(B) * J.PART * 4
    return dict(w, stride=(w["bytes"] + 255) // 256 * 256)


def test_sizes(lib):
    """F = 294, three members, B = 136 (two forward workgroups) and others: the stride is the single entry's bytes rounded
    up to 256 (an odd B's dh [B][32] is no multiple of 256 bytes), the workspace three strides."""
    single, one_launches = C.c_size_t(), C.c_int32()
    for B in (136, 33, 1, 48, 264, 512):
        assert lib.antsrl_jointtrain_sizes(294, B, None, C.byref(single), C.byref(one_launches)) == 0
        want = member_layout(B)
        assert single.value == want["bytes"]
        rc, tf, stride, ws, n = sizes(lib, 294, B, 3)
        assert rc == 0 and tf == 32 * 296 + 230
        assert stride == want["stride"] and stride % 256 == 0 and single.value <= stride < single.value + 256, (B, stride)
        assert ws == 3 * stride and n == 2 == one_launches.value
    assert sizes(lib, 294, 33, 3)[2] > member_layout(33)["bytes"]  # B = 33: 33 * 128 is no multiple of 256, the stride is rounded
    assert [member_layout(B)["blocks"] for B in (1, 128, 129, 384, 385, 512)] == [1, 1, 2, 3, 4, 4]
    for F in (1, 9, 17, 609, 848, 1022):
        assert sizes(lib, F, 48, 64)[:2] == (0, 32 * (F + 2) + 230)
    assert sizes(lib, 294, 512, 64)[3] == 64 * member_layout(512)["stride"]
    # any output may be NULL
    assert lib.antsrl_pop_jointtrain_sizes(294, 136, 3, None, None, None, None) == 0


def test_stride_over_every_B(lib):
    """No B in [1, 512] gives a stride that is short of the member's partials and dh or no multiple of 256."""
    for B in range(1, 513):
        rc, _, stride, ws, _ = sizes(lib, 17, B, 2)
        want = member_layout(B)
        assert rc == 0 and stride == want["stride"] >= want["bytes"] and stride % 256 == 0 and ws == 2 * stride, B


@pytest.mark.parametrize("args,code,msg", [
    ((294, 0, 3), -1, b"B must be >= 1 (0)"), ((294, 513, 3), -4, b"B = 513 > 512 rows"),
    ((294, 48, 0), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    ((294, 48, 65), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    ((0, 48, 3), -1, b"n_features must be >= 1"), ((1023, 48, 3), -4, b"n_features + 2 = 1025 > 1024")])
def test_sizes_validation(lib, args, code, msg):
    assert sizes(lib, *args)[0] == code
    assert msg in lib.antsrl_last_error() and b"pop_jointtrain_sizes" in lib.antsrl_last_error(), lib.antsrl_last_error()


# ---- the training step
def test_train_B(lib):
    assert train(lib, spec(), B=513) == -4
    err = lib.antsrl_last_error()
    assert b"B = 513 > 512 rows" in err and b"pop_jointtrain_step" in err and b"at most four forward workgroups" in err, err
    assert train(lib, spec(), B=0) == -1 and b"B must be >= 1" in lib.antsrl_last_error()
    # 512 rows pass: the next refusal is a pointer's
    assert train(lib, spec(), B=512, model=None) == -1 and b"model is required" in lib.antsrl_last_error()


def test_train_n_members(lib):
    for P in (0, 65):
        assert train(lib, spec(P=P, E=max(P, 1))) == -1
        assert b"n_members must be in [1, ANTSRL_POP_MAX = 64] (%d)" % P in lib.antsrl_last_error()
    # 64 members pass: the next refusal is a pointer's
    assert train(lib, spec(P=64, E=64), model=None) == -1 and b"model is required" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in TRAIN_PTRS] + [
    ({n: ODD}, n.encode() + b" must be") for n in TRAIN_PTRS if n != "dones"] + [
    (dict(idx=None), b"idx is required"), (dict(idx=ODD4), b"idx must be 8-byte"), (dict(loss=None), b"loss is required"),
    (dict(loss=ODD), b"loss must be 4-byte"), (dict(grads=ODD), b"grads must be 4-byte"),
    (dict(running_loss=ODD4), b"running_loss must be 8-byte"), (dict(workspace=None), b"workspace is required"),
    (dict(workspace=ODD128), b"workspace must be 256-byte"), (dict(n_rows=0), b"n_rows"),
    (dict(step=0), b"step must be >= 1"), (dict(beta1=1.0), b"beta1, beta2"), (dict(eps=0.0), b"eps must be")])
def test_train_validation(lib, kw, msg):
    assert train(lib, spec(), **kw) == -1, kw
    assert msg in lib.antsrl_last_error() and b"pop_jointtrain_step" in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


def test_train_member_learning_rate(lib):
    s = spec()
    s.members[2].learning_rate = -1.0
    assert train(lib, s) == -1 and b"lr must be" in lib.antsrl_last_error()
