"""CPU-side checks of the memory agent's C-ABI entries (antsrl_agent_select, antsrl_replay_record_pre / _post): exported,
the ctypes AntsRecordSpec has the C struct's layout, and every invalid argument is refused with a message before any HIP
call.  No kernel is launched here: every call below fails validation, and the pointers are fakes that are never
dereferenced."""
import ctypes as C

import pytest

from abi_fakes import FAKE, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_agent_select", "antsrl_replay_record_pre", "antsrl_replay_record_post")
FAKE2 = C.c_void_p(1 << 30)


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.antsrl_abi_version() == 5


def test_record_spec_layout():
    """include/antsrl.h: ten int32, then K, head, max_len (int64) and seed, step (uint64), no padding: 80 bytes."""
    S = _lib.AntsRecordSpec
    assert C.sizeof(S) == 80
    assert [getattr(S, n).offset for n in ("n_envs", "n_ants", "env_id_base", "n_features", "agent_dim", "mem_size", "n_rot",
                                          "obs_format", "obs_pitch", "reserved")] == list(range(0, 40, 4))
    assert [getattr(S, n).offset for n in ("K", "head", "max_len", "seed", "step")] == [40, 48, 56, 64, 72]


def select(lib, **kw):
    a = dict(seed=1, step=0, base=0, E=4, N=64, eps=0.5, n_rot=3, n_ph=3, mem=20, rot=FAKE, ph=FAKE, old=FAKE, new=FAKE2,
             explored=None)
    a.update(kw)
    return lib.antsrl_agent_select(a["seed"], a["step"], a["base"], a["E"], a["N"], a["eps"], a["n_rot"], a["n_ph"], a["mem"],
                                   a["rot"], a["ph"], a["old"], a["new"], a["explored"], None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(E=0), -1, b"n_envs"), (dict(N=0), -1, b"n_ants"), (dict(E=-3), -1, b"n_envs"),
    (dict(E=1 << 16, N=1 << 15), -1, b"2^31"), (dict(base=-1), -1, b"env_id_base"),
    (dict(base=0x7fffffff), -1, b"env_id_base"),
    (dict(eps=-0.01), -1, b"epsilon"), (dict(eps=1.01), -1, b"epsilon"), (dict(eps=float("nan")), -1, b"epsilon"),
    (dict(n_rot=0), -1, b"n_rot"), (dict(n_rot=33), -4, b"n_rot"), (dict(n_ph=0), -1, b"n_ph"), (dict(n_ph=33), -4, b"n_ph"),
    (dict(mem=0), -1, b"mem_size"), (dict(mem=33), -4, b"mem_size"),
    (dict(rot=None), -1, b"rotation"), (dict(ph=None), -1, b"pheromone"), (dict(old=None), -1, b"mem_old"),
    (dict(new=None), -1, b"mem_next"), (dict(old=C.c_void_p((1 << 20) + 2)), -1, b"4-byte"),
    (dict(new=C.c_void_p((1 << 20) + 64)), -1, b"overlap"),
])
def test_select_validation(lib, kw, code, msg):
    assert select(lib, **kw) == code, kw
    assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


def spec(**kw):
    a = dict(n_envs=4, n_ants=64, env_id_base=0, n_features=294, agent_dim=2, mem_size=20, n_rot=3, obs_format=0,
             obs_pitch=0, reserved=0, K=256, head=0, max_len=1000, seed=1, step=0)
    a.update(kw)
    return _lib.AntsRecordSpec(**a)


def pre(lib, s, **kw):
    a = dict(obs=FAKE, ast=FAKE, mem=FAKE, rot=FAKE, ph=FAKE, states=FAKE, agent_states=FAKE, actions=FAKE)
    a.update(kw)
    return lib.antsrl_replay_record_pre(C.byref(s) if s is not None else None, a["obs"], a["ast"], a["mem"], a["rot"], a["ph"],
                                        a["states"], a["agent_states"], a["actions"], None)


def post(lib, s, **kw):
    a = dict(obs=FAKE, ast=FAKE, mem=FAKE, reward=FAKE, done=FAKE, rewards=FAKE, new_states=FAKE, new_agent_states=FAKE,
             dones=FAKE)
    a.update(kw)
    return lib.antsrl_replay_record_post(C.byref(s) if s is not None else None, a["obs"], a["ast"], a["mem"], a["reward"],
                                         a["done"], a["rewards"], a["new_states"], a["new_agent_states"], a["dones"], None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(n_envs=0), -1, b"n_envs"), (dict(n_ants=0), -1, b"n_ants"), (dict(n_envs=1 << 16, n_ants=1 << 15), -1, b"2^31"),
    (dict(env_id_base=-1), -1, b"env_id_base"),
    (dict(K=0), -1, b"K must be"), (dict(K=257), -1, b"K must be"), (dict(K=-1), -1, b"K must be"),
    (dict(max_len=0), -1, b"max_len"), (dict(head=-1), -1, b"head"), (dict(head=1000), -1, b"head"),
    (dict(obs_format=2), -1, b"obs_format"), (dict(obs_format=-1), -1, b"obs_format"),
    (dict(obs_pitch=293), -1, b"obs_pitch"), (dict(obs_pitch=-8), -1, b"obs_pitch"),
    (dict(n_features=0), -1, b"n_features"), (dict(n_features=1003), -4, b"1024"),
    (dict(agent_dim=0), -1, b"agent_dim"), (dict(agent_dim=33), -4, b"agent_dim"),
    (dict(mem_size=0), -1, b"mem_size"), (dict(mem_size=33), -4, b"mem_size"),
    (dict(n_rot=0), -1, b"n_rot"), (dict(n_rot=33), -4, b"n_rot"),
])
def test_record_spec_validation(lib, kw, code, msg):
    s = spec(**kw)
    for call in (pre, post):
        assert call(lib, s) == code, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


def test_record_pointer_validation(lib):
    s = spec()
    assert pre(lib, None) == -1 and b"NULL spec" in lib.antsrl_last_error()
    assert post(lib, None) == -1 and b"NULL spec" in lib.antsrl_last_error()
    odd = C.c_void_p((1 << 20) + 2)
    for kw, msg in ((dict(obs=None), b"obs"), (dict(ast=None), b"agent_state"), (dict(mem=None), b"memory"),
                    (dict(rot=None), b"rotation"), (dict(states=None), b"states"), (dict(agent_states=None), b"agent_states"),
                    (dict(actions=None), b"actions"), (dict(obs=odd), b"4-byte"), (dict(states=odd), b"4-byte"),
                    (dict(actions=C.c_void_p((1 << 20) + 4)), b"8-byte")):
        assert pre(lib, s, **kw) == -1, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    for kw, msg in ((dict(obs=None), b"obs"), (dict(ast=None), b"agent_state"), (dict(mem=None), b"memory"),
                    (dict(reward=None), b"reward"), (dict(done=None), b"done"), (dict(rewards=None), b"rewards"),
                    (dict(new_states=None), b"new_states"), (dict(new_agent_states=None), b"new_agent_states"),
                    (dict(dones=None), b"dones"), (dict(reward=odd), b"4-byte")):
        assert post(lib, s, **kw) == -1, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    # bfloat16 observations need 2-byte alignment only; an odd address is refused
    b = spec(obs_format=1)
    assert pre(lib, b, obs=C.c_void_p((1 << 20) + 1)) == -1 and b"2-byte" in lib.antsrl_last_error()
