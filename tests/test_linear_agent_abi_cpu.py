"""CPU-side checks of the linear agent's C-ABI entries (antsrl_agent_select_actions, antsrl_replay_record_pre_plain /
_post_plain, antsrl_lintrain_sizes / _grad / _apply / _step): exported, and every invalid
argument refused with a message before any HIP call.  No kernel is launched here: every call below fails validation (or
is antsrl_lintrain_sizes, which is host arithmetic), and the pointers are fakes that are never dereferenced."""
import ctypes as C

import pytest

import train_abi as TA
from abi_fakes import FAKE, ODD, ODD4, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_agent_select_actions", "antsrl_replay_record_pre_plain", "antsrl_replay_record_post_plain",
       "antsrl_lintrain_sizes", "antsrl_lintrain_grad", "antsrl_lintrain_apply", "antsrl_lintrain_step")


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.antsrl_abi_version() == 5


def select(lib, **kw):
    a = dict(seed=1, step=0, base=0, E=4, N=64, eps=0.5, n_rot=3, n_ph=3, rot=FAKE, ph=FAKE, explored=None)
    a.update(kw)
    return lib.antsrl_agent_select_actions(a["seed"], a["step"], a["base"], a["E"], a["N"], a["eps"], a["n_rot"], a["n_ph"],
                                           a["rot"], a["ph"], a["explored"], None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(E=0), -1, b"n_envs"), (dict(N=0), -1, b"n_ants"), (dict(E=1 << 16, N=1 << 15), -1, b"2^31"),
    (dict(base=-1), -1, b"env_id_base"), (dict(base=0x7fffffff), -1, b"env_id_base"),
    (dict(eps=-0.01), -1, b"epsilon"), (dict(eps=1.01), -1, b"epsilon"), (dict(eps=float("nan")), -1, b"epsilon"),
    (dict(n_rot=0), -1, b"n_rot"), (dict(n_rot=33), -4, b"n_rot"), (dict(n_ph=0), -1, b"n_ph"), (dict(n_ph=33), -4, b"n_ph"),
    (dict(rot=None), -1, b"rotation"), (dict(ph=None), -1, b"pheromone"),
])
def test_select_actions_validation(lib, kw, code, msg):
    assert select(lib, **kw) == code, kw
    err = lib.antsrl_last_error()
    assert msg in err and b"agent_select_actions" in err, (kw, err)


def spec(**kw):
    a = dict(n_envs=4, n_ants=64, env_id_base=0, n_features=294, agent_dim=2, mem_size=0, n_rot=3, obs_format=0, obs_pitch=0,
             reserved=0, K=256, head=0, max_len=1000, seed=1, step=0)
    a.update(kw)
    return _lib.AntsRecordSpec(*[a[n] for n, _ in _lib.AntsRecordSpec._fields_])


SPEC_CASES = [
    (dict(mem_size=20), -1, b"mem_size must be 0"), (dict(mem_size=-1), -1, b"mem_size must be 0"),
    (dict(n_envs=0), -1, b"n_envs"), (dict(n_ants=0), -1, b"n_ants"), (dict(env_id_base=-1), -1, b"env_id_base"),
    (dict(n_features=0), -1, b"n_features"), (dict(agent_dim=0), -1, b"agent_dim"), (dict(agent_dim=33), -4, b"agent_dim"),
    (dict(n_rot=0), -1, b"n_rot"), (dict(n_features=1023), -4, b"1024"), (dict(obs_format=2), -1, b"obs_format"),
    (dict(obs_pitch=100), -1, b"obs_pitch"), (dict(K=0), -1, b"K must be in [1"), (dict(K=257), -1, b"K must be in [1"),
    (dict(max_len=0), -1, b"max_len"), (dict(head=-1), -1, b"head"), (dict(head=1000), -1, b"head"),
]


def pre(lib, s, **kw):
    a = dict(obs=FAKE, ast=FAKE, rot=FAKE, ph=FAKE, states=FAKE, asts=FAKE, actions=FAKE)
    a.update(kw)
    return lib.antsrl_replay_record_pre_plain(C.byref(s) if s is not None else None, a["obs"], a["ast"], a["rot"], a["ph"],
                                              a["states"], a["asts"], a["actions"], None)


def post(lib, s, **kw):
    a = dict(obs=FAKE, ast=FAKE, reward=FAKE, done=FAKE, rewards=FAKE, nst=FAKE, nast=FAKE, dones=FAKE)
    a.update(kw)
    return lib.antsrl_replay_record_post_plain(C.byref(s) if s is not None else None, a["obs"], a["ast"], a["reward"],
                                               a["done"], a["rewards"], a["nst"], a["nast"], a["dones"], None)


@pytest.mark.parametrize("kw,code,msg", SPEC_CASES)
def test_record_plain_spec_validation(lib, kw, code, msg):
    for fn, who in ((pre, b"replay_record_pre_plain"), (post, b"replay_record_post_plain")):
        assert fn(lib, spec(**kw)) == code, kw
        err = lib.antsrl_last_error()
        assert msg in err and who in err, (kw, err)


def test_record_plain_null_spec(lib):
    assert pre(lib, None) == -1 and b"NULL spec" in lib.antsrl_last_error()
    assert post(lib, None) == -1 and b"NULL spec" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(obs=None), b"obs is required"), (dict(ast=None), b"agent_state is required"), (dict(rot=None), b"rotation is required"),
    (dict(states=None), b"states is required"), (dict(asts=None), b"agent_states is required"),
    (dict(actions=None), b"actions is required"), (dict(obs=ODD), b"obs must be 4-byte"), (dict(states=ODD), b"states must be 4-byte"),
    (dict(actions=ODD4), b"actions must be 8-byte"),
])
def test_record_pre_plain_pointers(lib, kw, msg):
    assert pre(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error(), lib.antsrl_last_error()


def test_record_pre_plain_bf16_alignment(lib):
    assert pre(lib, spec(obs_format=1), obs=C.c_void_p((1 << 20) + 1)) == -1
    assert b"obs must be 2-byte" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(obs=None), b"obs is required"), (dict(ast=None), b"agent_state is required"), (dict(reward=None), b"reward is required"),
    (dict(done=None), b"done is required"), (dict(rewards=None), b"rewards is required"), (dict(nst=None), b"new_states is required"),
    (dict(nast=None), b"new_agent_states is required"), (dict(dones=None), b"dones is required"),
    (dict(reward=ODD), b"reward must be 4-byte"), (dict(nst=ODD), b"new_states must be 4-byte"),
])
def test_record_post_plain_pointers(lib, kw, msg):
    assert post(lib, spec(), **kw) == -1
    assert msg in lib.antsrl_last_error(), lib.antsrl_last_error()


# ---- the training step
def test_lintrain_sizes(lib):
    tf, ws, n = C.c_size_t(), C.c_size_t(), C.c_int32()
    assert lib.antsrl_lintrain_sizes(294, 264, C.byref(tf), C.byref(ws), C.byref(n)) == 0
    assert tf.value == 198 and n.value == 1          # the reference's minibatch: one launch
    assert lib.antsrl_lintrain_sizes(294, 512, None, None, C.byref(n)) == 0 and n.value == 1
    assert lib.antsrl_lintrain_sizes(294, 513, None, C.byref(ws), C.byref(n)) == 0 and n.value == 2
    assert ws.value == 5 * 200 * 4                   # 17 tiles: 5 workgroups of 4 waves
    assert lib.antsrl_lintrain_sizes(294, 1 << 24, None, C.byref(ws), C.byref(n)) == 0 and n.value == 2
    assert ws.value == 1024 * 200 * 4
    for F, B, code, msg in ((0, 264, -1, b"n_features"), (1023, 264, -4, b"1024"), (294, 0, -1, b"B must be"),
                            (294, (1 << 24) + 1, -1, b"B must be")):
        assert lib.antsrl_lintrain_sizes(F, B, None, None, None) == code
        assert msg in lib.antsrl_last_error()


# the step's entries through train_abi.Kind; the cases are this file's own: B's limit is an INVALID one, the workspace is
# needed beyond one workgroup only, and the step's default has no grads
KIND = TA.Kind("lintrain", ("w1", "b1", "heads", "target_l3"), lambda a: a["F"], ("heads",),
               dict(F=294, B=264, work=C.c_void_p(1 << 21)), step_defaults=dict(grads=None))

BATCH_CASES = [(dict(F=0), -1, b"n_features"), (dict(F=1023), -4, b"1024"), (dict(B=0), -1, b"B must be"),
               (dict(B=(1 << 24) + 1), -1, b"B must be"), (dict(n_rows=0), -1, b"n_rows"),
               (dict(idx=None, B=264, n_rows=100), -1, b"without idx"), (dict(idx=ODD4), -1, b"idx must be 8-byte"),
               (dict(actions=ODD4), -1, b"actions must be 8-byte"), (dict(loss=None), -1, b"loss is required"),
               (dict(loss=ODD), -1, b"loss must be 4-byte"), (dict(discount=float("nan")), -1, b"discount is NaN"),
               (dict(B=4096, work=None), -1, b"workspace is required"),
               (dict(B=4096, work=C.c_void_p((1 << 21) + 16)), -1, b"workspace must be 256-byte"),
               (dict(grads=ODD), -1, b"grads must be 4-byte")] + TA.pointer_cases(KIND.ptrs)


@pytest.mark.parametrize("kw,code,msg", BATCH_CASES)
def test_lintrain_grad_and_step_validation(lib, kw, code, msg):
    KIND.check(("grad", "step"), lib, kw, code, msg)


def test_lintrain_grad_needs_grads(lib):
    KIND.check_grad_needs_grads(lib)


ADAM_CASES = [(dict(step=0), b"step must be >= 1"), (dict(lr=-1.0), b"lr must be"), (dict(lr=float("inf")), b"lr must be"),
              (dict(beta1=1.0), b"beta1, beta2"), (dict(beta2=-0.1), b"beta1, beta2"), (dict(eps=0.0), b"eps must be"),
              (dict(eps=float("nan")), b"eps must be")]


@pytest.mark.parametrize("kw,msg", ADAM_CASES + [(dict(m=None), b"adam_m is required"), (dict(v=ODD), b"adam_v must be 4-byte")])
def test_lintrain_step_adam_validation(lib, kw, msg):
    KIND.check(("step",), lib, kw, -1, msg)


@pytest.mark.parametrize("kw,msg", ADAM_CASES + [(dict(heads=None), b"heads is required"), (dict(m=None), b"adam_m is required"),
                                                 (dict(v=None), b"adam_v is required"), (dict(grads=None), b"grads is required"),
                                                 (dict(heads=ODD), b"heads must be 4-byte")])
def test_lintrain_apply_validation(lib, kw, msg):
    KIND.check(("apply",), lib, kw, -1, msg)
