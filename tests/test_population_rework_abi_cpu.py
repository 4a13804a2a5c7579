"""CPU-side checks of the rework population's C-ABI entries (antsrl_pop_rework_collapse / antsrl_pop_policy_rework /
antsrl_pop_policy_rework_select / antsrl_pop_reworktrain_sizes / antsrl_pop_reworktrain_step; include/antsrl.h, "The
population of rework agents"): exported, the sizes against the single agent's antsrl_reworktrain_sizes, and every invalid
argument refused in its own words before any HIP call.  No kernel is launched here: every call of an enqueueing entry
fails validation, and the pointers are fakes that are never dereferenced (tests/test_population_explore_abi_cpu.py's
way)."""
import ctypes as C

import pytest

from abi_fakes import FAKE, ODD, ODD4, ODD8, ODD128, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib
from population_abi import TRAIN_TAIL, spec

NEW = ("antsrl_pop_rework_collapse", "antsrl_pop_policy_rework", "antsrl_pop_policy_rework_select",
       "antsrl_pop_reworktrain_sizes", "antsrl_pop_reworktrain_step")


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS, n
    assert lib.antsrl_abi_version() == 5  # the entries are additive


def rshape(**kw):
    """The reference's CollectModelRework at F = 294 unless a field is given."""
    a = dict(n_features=294, agent_dim=2, g1=64, g2=128, g3=32, r1=64, r2=128, r3=32, p1=32, n_rot=3, n_ph=3)
    a.update(kw)
    return _lib.AntsReworkShape(*[a[n] for n, _ in _lib.AntsReworkShape._fields_])


def ref(x):
    return C.byref(x) if x is not None else None


POLICY_PTRS = ("collapsed", "obs", "agent_state", "rotation", "pheromone", "q_out")
SELECT_ORDER = ("collapsed", "obs", "agent_state", "step", "rotation", "pheromone", "explored", "q_out")
TRAIN_PTRS = ("model", "target_collapsed", "adam_m", "adam_v", "states", "agent_states", "actions", "rewards", "new_states",
              "new_agent_states", "dones")


def policy(lib, s, shp=None, null_shape=False, **kw):
    a = dict({n: FAKE for n in POLICY_PTRS}, **kw)
    shp = None if null_shape else (shp or rshape())
    return lib.antsrl_pop_policy_rework(ref(s), ref(shp), *[a[n] for n in POLICY_PTRS], None)


def select(lib, s, shp=None, null_shape=False, **kw):
    a = dict({n: FAKE for n in SELECT_ORDER}, step=3, **kw)
    shp = None if null_shape else (shp or rshape())
    return lib.antsrl_pop_policy_rework_select(ref(s), ref(shp), *[a[n] for n in SELECT_ORDER], None)


def train(lib, s, shp=None, null_shape=False, **kw):
    order = TRAIN_PTRS + tuple(TRAIN_TAIL) + ("workspace",)
    a = dict({n: FAKE for n in TRAIN_PTRS}, **TRAIN_TAIL, workspace=FAKE)
    a.update(kw)
    shp = None if null_shape else (shp or rshape())
    return lib.antsrl_pop_reworktrain_step(ref(s), ref(shp), *[a[n] for n in order], None)


def collapse(lib, shp, P=3, blocks=FAKE, collapsed=FAKE):
    return lib.antsrl_pop_rework_collapse(ref(shp), P, blocks, collapsed, None)


def sizes(lib, shp, B, P):
    tf, cf, stride, ws, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = lib.antsrl_pop_reworktrain_sizes(ref(shp), B, P, C.byref(tf), C.byref(cf), C.byref(stride), C.byref(ws), C.byref(n))
    return rc, tf.value, cf.value, stride.value, ws.value, n.value


def single_sizes(lib, shp, B):
    pf, ws, n = C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = lib.antsrl_reworktrain_sizes(ref(shp), B, C.byref(pf), C.byref(ws), C.byref(n))
    return rc, pf.value, ws.value, n.value


ENTRIES = ((policy, b"pop_policy_rework"), (select, b"pop_policy_rework_select"), (train, b"pop_reworktrain_step"))


# ---- the spec: the three enqueueing entries refuse it in the linear population's words, under their own names
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
        assert msg in err and who + b":" in err, (kw, err)


def test_null_spec_and_shape(lib):
    for fn, who in ENTRIES:
        assert fn(lib, None) == -1
        assert b"NULL spec" in lib.antsrl_last_error() and who + b":" in lib.antsrl_last_error()
        assert fn(lib, spec(), null_shape=True) == -1
        assert b"NULL shape" in lib.antsrl_last_error() and who + b":" in lib.antsrl_last_error()
    assert collapse(lib, None) == -1 and b"pop_rework_collapse: NULL shape" in lib.antsrl_last_error()
    assert sizes(lib, None, 48, 3)[0] == -1 and b"pop_reworktrain_sizes: NULL shape" in lib.antsrl_last_error()


# ---- the shape: antsrl_rework_collapse's rules, in its words, under every entry's name
SHAPE_CASES = [
    (dict(n_rot=0), -1, b"n_features, agent_dim, n_rot, n_ph must be >= 1"),
    (dict(n_ph=0), -1, b"n_features, agent_dim, n_rot, n_ph must be >= 1"),
    (dict(n_rot=9), -4, b"n_rot, n_ph (9, 3) must be <= 8"), (dict(n_ph=9), -4, b"n_rot, n_ph (3, 9) must be <= 8"),
    (dict(g2=0), -1, b"g2 must be >= 1 (0)"), (dict(r3=257), -4, b"r3 257 > 256"),
    (dict(agent_dim=3), -4, b"agent_dim 3 is not 2"),
]


@pytest.mark.parametrize("kw,code,msg", SHAPE_CASES)
def test_shape_validation(lib, kw, code, msg):
    shp = rshape(**kw)
    calls = [(lambda fn=fn: fn(lib, spec(), shp), who) for fn, who in ENTRIES]
    calls += [(lambda: collapse(lib, shp), b"pop_rework_collapse"), (lambda: sizes(lib, shp, 48, 3)[0], b"pop_reworktrain_sizes")]
    for fn, who in calls:
        assert fn() == code, (who, kw)
        err = lib.antsrl_last_error()
        assert msg in err and who + b":" in err, (kw, err)


def test_shape_too_wide(lib):
    """D = n_features + 2 > 1024 is the shape's refusal where no spec is in front of it."""
    shp = rshape(n_features=1023)
    assert collapse(lib, shp) == -4 and b"D = n_features + agent_dim = 1025 > 1024" in lib.antsrl_last_error()
    assert sizes(lib, shp, 48, 3)[0] == -4 and b"D = n_features + agent_dim = 1025 > 1024" in lib.antsrl_last_error()


def test_spec_and_shape_speak_of_the_same_rows(lib):
    for fn, who in ENTRIES:
        assert fn(lib, spec(F=294), rshape(n_features=50)) == -1
        err = lib.antsrl_last_error()
        assert b"the spec's n_features = 294 is not the shape's 50" in err and who + b":" in err, err


# ---- the acting entries
def test_policy_alignment_rule(lib):
    """Em = 1, n_ants = 33, F = 294, bfloat16: a member's slice is 19 404 bytes = 16 * 1212 + 12."""
    for fn, who in ENTRIES[:2]:
        assert fn(lib, spec(P=2, E=2, N=33, fmt=1)) == -4
        err = lib.antsrl_last_error()
        assert who + b":" in err and b"19404 bytes" in err and b"multiple of 16" in err, err
        # the acceptance test's two shapes pass the rule: what is refused next is a pointer
        for s in (spec(P=3, E=6, N=20, fmt=1), spec(P=2, E=2, N=32, fmt=0)):
            assert fn(lib, s, collapsed=None) == -1 and b"collapsed is required" in lib.antsrl_last_error()
    # F = 1000 is no flat-form refusal here: the rework net acts up to D = 1024 (the next refusal is a pointer's)
    assert policy(lib, spec(F=1000, N=32, fmt=0), rshape(n_features=1000), obs=None) == -1
    assert b"obs is required" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [({n: None}, n.encode() + b" is required") for n in POLICY_PTRS if n != "q_out"] + [
    (dict(collapsed=ODD), b"collapsed must be 4-byte"), (dict(obs=ODD8), b"obs must be 16-byte"),
    (dict(agent_state=ODD), b"agent_state must be 4-byte"), (dict(q_out=ODD), b"q_out must be 4-byte")])
def test_policy_pointers(lib, kw, msg):
    for fn, who in ENTRIES[:2]:
        assert fn(lib, spec(), **kw) == -1, (who, kw)
        assert msg in lib.antsrl_last_error() and who + b":" in lib.antsrl_last_error(), lib.antsrl_last_error()


def test_collapse_arguments(lib):
    for P in (0, 65):
        assert collapse(lib, rshape(), P=P) == -1
        assert b"pop_rework_collapse: n_members must be in [1, ANTSRL_POP_MAX = 64] (%d)" % P in lib.antsrl_last_error()
    for kw, msg in ((dict(blocks=None), b"target_blocks is required"), (dict(blocks=ODD), b"target_blocks must be 4-byte"),
                    (dict(collapsed=None), b"collapsed is required"), (dict(collapsed=ODD), b"collapsed must be 4-byte")):
        assert collapse(lib, rshape(), **kw) == -1 and msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


# ---- the sizes
def test_sizes_for_one_member_are_the_single_trainer_s(lib):
    for shp in (rshape(), rshape(n_features=50, n_rot=5, n_ph=4, g1=8, g2=16, g3=8, r1=8, r2=16, r3=8, p1=8), rshape(n_features=1022, n_rot=8, n_ph=8)):
        D, NQ = shp.n_features + 2, shp.n_rot + shp.n_ph
        for B in (1, 40, 264, 4112):
            one = single_sizes(lib, shp, B)
            rc, tf, cf, stride, ws, n = sizes(lib, shp, B, 1)
            assert rc == 0 == one[0] and tf == one[1] and n == 4 == one[3]
            assert cf == NQ * D + NQ and stride % 256 == 0 and one[2] <= stride < one[2] + 256 and ws == stride
            assert sizes(lib, shp, B, 64)[1:] == (tf, cf, stride, 64 * stride, 4)
    assert sizes(lib, rshape(), 264, 3)[1:3] == (82382, 1782)  # the reference's net: neither count is a multiple of 4
    assert lib.antsrl_pop_reworktrain_sizes(C.byref(rshape()), 264, 3, None, None, None, None, None) == 0  # any output may be NULL


def test_stride_over_every_B(lib):
    """No B in [1, 600] or at the seams of the partials (4096 rows fill 256 parts, 4097 loop) or at the limit gives a
    stride that is short of the single step's workspace or no multiple of 256."""
    shp = rshape(n_features=17)
    for B in list(range(1, 601)) + [4096, 4097, 65536]:
        rc, _, _, stride, ws, _ = sizes(lib, shp, B, 2)
        one = single_sizes(lib, shp, B)
        assert rc == 0 == one[0] and stride % 256 == 0 and stride >= one[2] and ws == 2 * stride, B
    assert sizes(lib, shp, 65537, 2)[0] == -4
    assert b"pop_reworktrain_sizes: B = 65537 > 65536 rows" in lib.antsrl_last_error()


@pytest.mark.parametrize("args,code,msg", [
    ((0, 3), -1, b"B must be >= 1 (0)"), ((65537, 3), -4, b"B = 65537 > 65536 rows"),
    ((48, 0), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    ((48, 65), -1, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (65)")])
def test_sizes_validation(lib, args, code, msg):
    assert sizes(lib, rshape(), *args)[0] == code
    assert msg in lib.antsrl_last_error() and b"pop_reworktrain_sizes:" in lib.antsrl_last_error(), lib.antsrl_last_error()


# ---- the training step
def test_train_B(lib):
    assert train(lib, spec(), B=65537) == -4
    assert b"pop_reworktrain_step: B = 65537 > 65536 rows" in lib.antsrl_last_error()
    assert train(lib, spec(), B=0) == -1 and b"B must be >= 1" in lib.antsrl_last_error()
    # 65536 rows pass: the next refusal is a pointer's
    assert train(lib, spec(), B=65536, model=None) == -1 and b"model is required" in lib.antsrl_last_error()


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
    assert msg in lib.antsrl_last_error() and b"pop_reworktrain_step:" in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


def test_train_member_learning_rate(lib):
    """As the neighbours treat it: a member's negative or NaN learning rate is Adam's refusal; 0 is a step size of 0 and
    passes (every argument was valid: nothing is left to refuse, so the call is not made here)."""
    for bad in (-1.0, float("nan")):
        s = spec()
        s.members[2].learning_rate = bad
        assert train(lib, s) == -1 and b"pop_reworktrain_step: lr must be" in lib.antsrl_last_error()
