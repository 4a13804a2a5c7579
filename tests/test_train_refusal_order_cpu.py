"""Which refusal wins: the order in which the explore and the joint step's C-ABI entries, single and population, check
their arguments (antsrl_{exptrain,jointtrain}_{sizes,grad,apply,step}, antsrl_pop_{exptrain,jointtrain}_{sizes,step},
antsrl_pop_explore_policy, antsrl_pop_joint_policy).  The *_abi_cpu.py files pin every refusal alone; here ORDER lists an
entry's checked arguments in the order the entry refuses them, each with one bad value and the code and words of its
refusal, and call j makes arguments j .. n bad and 1 .. j - 1 good: it must be refused in the words of argument j.

No call has every argument good, so none passes validation: nothing is launched, and the pointers are fakes that are
never dereferenced.  An argument an entry checks twice (n_features: its range, then whether the acting net fits the LDS)
stands twice, the second time with a value that passes the first check."""
import ctypes as C

import pytest

import train_abi as TA
from abi_fakes import FAKE, INVALID, ODD, ODD4, UNSUPPORTED, lib  # noqa: F401 (lib is a fixture)
from population_abi import TRAIN_TAIL, call, spec

NAN = float("nan")


def ptr(name, abi=None):
    return (name, {}, {name: None}, INVALID, (abi or name).encode() + b" is required")


# ---- the single steps: (label, {}, bad keywords of train_abi.Kind, code, words)
FEATURES = ("n_features", {}, dict(F=0), INVALID, b"n_features must be >= 1")
ROWS = ("B", {}, dict(B=0), INVALID, b"B must be >= 1")
ADAM = [("step", {}, dict(step=0), INVALID, b"step must be >= 1"), ("lr", {}, dict(lr=-1.0), INVALID, b"lr must be"),
        ("beta1", {}, dict(beta1=1.0), INVALID, b"beta1, beta2 must be"), ("beta2", {}, dict(beta2=-0.1), INVALID, b"beta1, beta2 must be"),
        ("eps", {}, dict(eps=0.0), INVALID, b"eps must be")]


def minibatch(grads):
    return [("n_rows", {}, dict(n_rows=0), INVALID, b"n_rows must be")] + [ptr(n) for n in TA.ARRAYS] + [
        ("idx", {}, dict(idx=ODD4), INVALID, b"idx must be 8-byte aligned"), grads, ptr("loss")]


def single(target):
    net = [FEATURES, ROWS, ptr("model"), ptr(target), ptr("work", "workspace")]
    discount = ("discount", {}, dict(discount=NAN), INVALID, b"discount is NaN")
    return dict(
        sizes=[FEATURES, ROWS],
        grad=net + minibatch(ptr("grads")) + [discount],
        step=net + minibatch(("grads", {}, dict(grads=ODD), INVALID, b"grads must be 4-byte aligned")) + [discount]
        + [ptr("m", "adam_m"), ptr("v", "adam_v")] + ADAM,
        apply=[FEATURES, ptr("model"), ptr("m", "adam_m"), ptr("v", "adam_v"), ptr("grads")] + ADAM)


# ---- the populations: (label, bad keywords of population_abi.spec, bad keywords of the call, code, words)
SPEC = [("spec", dict(null=True), {}, INVALID, b"NULL spec"),
        ("n_members", dict(P=0), {}, INVALID, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
        ("n_envs", dict(E=0), {}, INVALID, b"n_envs and n_ants must be >= 1"),
        ("n_ants", dict(N=0), {}, INVALID, b"n_envs and n_ants must be >= 1"),
        ("env_id_base", dict(base=-1), {}, INVALID, b"env_id_base must be >= 0"),
        ("n_envs % n_members", dict(P=3, E=7), {}, INVALID, b"n_envs = 7 is not a multiple of n_members = 3"),
        ("n_features", dict(F=0), {}, INVALID, b"n_features must be >= 1"),
        ("obs_format", dict(fmt=2), {}, INVALID, b"obs_format must be"),
        ("obs_pitch", dict(pitch=320), {}, UNSUPPORTED, b"dense observation rows"),
        ("epsilon", dict(eps=1.5), {}, INVALID, b"member 0: epsilon must be in [0, 1]"),
        ("discount", dict(discount=NAN), {}, INVALID, b"member 0: discount is NaN")]


def pop_policy(net):
    return SPEC + [
        ("n_features fits", dict(F=1000), {}, UNSUPPORTED, b"flat form only"),
        # Em = 1, n_ants = 33, F = 294, bfloat16: a member's slice is 19 404 bytes = 16 * 1212 + 12
        ("slice bytes", dict(P=2, E=2, N=33, F=294, fmt=1), {}, UNSUPPORTED, b"multiple of 16"),
        ptr("obs"), ptr("agent_state")] + [ptr(n) for n in net]


def pop_step(target):
    return SPEC + [("B", {}, dict(B=0), INVALID, b"B must be >= 1")] + [
        ptr(n) for n in ("model", target, "adam_m", "adam_v", "idx", "workspace")] + [
        ("n_rows", {}, dict(n_rows=0), INVALID, b"n_rows must be")] + [ptr(n) for n in TA.ARRAYS] + [
        ("grads", {}, dict(grads=ODD), INVALID, b"grads must be 4-byte aligned"), ptr("loss"),
        ("running_loss", {}, dict(running_loss=ODD4), INVALID, b"running_loss must be 8-byte aligned"),
        ("step", {}, dict(step=0), INVALID, b"step must be >= 1"),
        ("learning_rate", dict(lr=-1.0), {}, INVALID, b"lr must be"),
        ("beta1", {}, dict(beta1=1.0), INVALID, b"beta1, beta2 must be"), ("beta2", {}, dict(beta2=-0.1), INVALID, b"beta1, beta2 must be"),
        ("eps", {}, dict(eps=0.0), INVALID, b"eps must be")]


POP_SIZES = [("n_features", {}, dict(F=0), INVALID, b"n_features must be >= 1"), ("B", {}, dict(B=0), INVALID, b"B must be >= 1"),
             ("n_members", {}, dict(P=0), INVALID, b"n_members must be in [1, ANTSRL_POP_MAX = 64] (0)")]

KINDS = dict(exptrain=TA.Kind("exptrain", ("model", "target"), lambda a: a["F"], ("lead", "model"), dict(F=294, B=256)),
             jointtrain=TA.Kind("jointtrain", ("model", "target_l3"), lambda a: a["F"], ("lead", "model"), dict(F=294, B=256)))


def call_single(entry, stage):
    def fn(lib, skw, kw):
        if stage == "sizes":
            a = dict(dict(F=294, B=256), **kw)
            return getattr(lib, "antsrl_%s_sizes" % entry)(a["F"], a["B"], None, None, None)
        return getattr(KINDS[entry], stage)(lib, **kw)
    return fn


def call_pop(entry, ptrs, tail=()):
    def fn(lib, skw, kw):
        s = None if skw.get("null") else spec(**{k: v for k, v in skw.items() if k != "null"})
        defaults = dict({n: FAKE for n in ptrs}, **dict(tail))
        return call(getattr(lib, "antsrl_" + entry), s, tuple(ptrs) + tuple(dict(tail)), defaults, kw)
    return fn


def call_pop_sizes(entry):
    def fn(lib, skw, kw):
        a = dict(dict(F=294, B=48, P=3), **kw)
        return getattr(lib, "antsrl_" + entry)(a["F"], a["B"], a["P"], None, None, None, None)
    return fn


ARRAYS = tuple(TA.ARRAYS)
EXPLORE_POLICY, JOINT_POLICY = ("target_blocks", "rotation"), ("model_blocks", "target_l3", "rotation", "pheromone")

#: entry -> (how to call it, its checked arguments in the order it refuses them)
ORDER = {}
for _entry, _target in (("exptrain", "target"), ("jointtrain", "target_l3")):
    for _stage, _items in single(_target).items():
        ORDER["%s_%s" % (_entry, _stage)] = (call_single(_entry, _stage), _items)
    ORDER["pop_%s_sizes" % _entry] = (call_pop_sizes("pop_%s_sizes" % _entry), POP_SIZES)
    ORDER["pop_%s_step" % _entry] = (call_pop("pop_%s_step" % _entry, ("model", _target, "adam_m", "adam_v") + ARRAYS,
                                              dict(TRAIN_TAIL, workspace=FAKE)), pop_step(_target))
ORDER["pop_explore_policy"] = (call_pop("pop_explore_policy", ("obs", "agent_state") + EXPLORE_POLICY), pop_policy(EXPLORE_POLICY))
ORDER["pop_joint_policy"] = (call_pop("pop_joint_policy", ("obs", "agent_state") + JOINT_POLICY), pop_policy(JOINT_POLICY))


def test_every_entry_is_listed():
    assert len(ORDER) == 14 and all(len(items) >= 2 for _, items in ORDER.values())


@pytest.mark.parametrize("entry,j", [(e, j) for e, (_, items) in ORDER.items() for j in range(len(items))])
def test_first_bad_argument_is_refused(lib, entry, j):
    fn, items = ORDER[entry]
    skw, kw = {}, {}
    for _, bad_spec, bad_kw, _, _ in reversed(items[j:]):  # (an argument listed twice: the earlier check's value holds)
        skw.update(bad_spec)
        kw.update(bad_kw)
    label, _, _, code, msg = items[j]
    assert fn(lib, skw, kw) == code, (entry, label)
    err = lib.antsrl_last_error()
    assert msg in err and entry.encode() + b":" in err, (entry, label, err)
