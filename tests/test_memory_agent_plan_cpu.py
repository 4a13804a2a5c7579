"""CPU-side checks of antsrl_agent_plan and antsrl_policy_memory_tiles: exported, every invalid argument refused with its
code and a message before any HIP call (the pointers are fakes that are never dereferenced), and the properties of the
plan's numpy restatement (tests/memory_agent_plan_ref.py) that the GPU tests hold the kernel to."""
import ctypes as C

import numpy as np
import pytest

import memory_agent_plan_ref as P
import memory_agent_ref as R
from abi_fakes import FAKE, ODD, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_agent_plan", "antsrl_policy_memory_tiles")


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert lib.antsrl_abi_version() == 5


def plan(lib, **kw):
    a = dict(seed=1, step=0, base=0, E=4, N=64, eps=0.5, tiles=FAKE, n_live=FAKE)
    a.update(kw)
    return lib.antsrl_agent_plan(a["seed"], a["step"], a["base"], a["E"], a["N"], a["eps"], a["tiles"], a["n_live"], None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(E=0), -1, b"n_envs"), (dict(N=0), -1, b"n_ants"), (dict(E=-3), -1, b"n_envs"), (dict(N=-1), -1, b"n_ants"),
    (dict(E=1 << 16, N=1 << 15), -1, b"2^31"), (dict(base=-1), -1, b"env_id_base"), (dict(base=0x7fffffff), -1, b"env_id_base"),
    (dict(eps=-0.01), -1, b"epsilon"), (dict(eps=1.01), -1, b"epsilon"), (dict(eps=float("nan")), -1, b"epsilon"),
    (dict(tiles=None), -1, b"tiles"), (dict(n_live=None), -1, b"n_live"),
    (dict(tiles=ODD), -1, b"4-byte"), (dict(n_live=ODD), -1, b"4-byte"),
])
def test_plan_validation(lib, kw, code, msg):
    assert plan(lib, **kw) == code, kw
    assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


def shape(**kw):
    a = dict(n_features=294, agent_dim=2, mem_size=20, h1=64, h2=128, h3=256, n_rot=3, n_ph=3)
    a.update(kw)
    return _lib.AntsMemNetShape(**a)


def forward(lib, s, **kw):
    a = dict(precision=0, packed=C.c_void_p(1 << 20), obs=FAKE, fmt=0, ast=FAKE, mem_in=FAKE, n_ants=64, mem_out=FAKE, rot=FAKE,
             tiles=FAKE, n_live=FAKE)
    a.update(kw)
    return lib.antsrl_policy_memory_tiles(C.byref(s) if s is not None else None, a["precision"], a["packed"], a["obs"], a["fmt"],
                                          a["ast"], a["mem_in"], a["n_ants"], a["mem_out"], a["rot"], None, None, a["tiles"],
                                          a["n_live"], None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(precision=2), -1, b"precision"), (dict(precision=-1), -1, b"precision"),
    (dict(fmt=2), -1, b"obs_format"), (dict(fmt=-1), -1, b"obs_format"),
    (dict(packed=None), -1, b"required"), (dict(obs=None), -1, b"required"), (dict(ast=None), -1, b"required"),
    (dict(mem_in=None), -1, b"required"), (dict(mem_out=None), -1, b"required"), (dict(rot=None), -1, b"required"),
    (dict(packed=C.c_void_p((1 << 20) + 64)), -1, b"256-byte"),
    (dict(tiles=None), -1, b"tiles and n_live"), (dict(n_live=None), -1, b"tiles and n_live"),
    (dict(tiles=ODD), -1, b"4-byte"), (dict(n_live=ODD), -1, b"4-byte"),
    (dict(n_ants=0), -1, b"n_ants"), (dict(n_ants=-5), -1, b"n_ants"), (dict(n_ants=1 << 31), -1, b"n_ants"),
])
def test_tiles_forward_validation(lib, kw, code, msg):
    for precision in (0, 1):
        a = dict(precision=precision)
        a.update(kw)
        assert forward(lib, shape(), **a) == code, a
        assert msg in lib.antsrl_last_error(), (a, lib.antsrl_last_error())


@pytest.mark.parametrize("kw,code,msg", [
    (dict(n_features=0), -1, b">= 1"), (dict(mem_size=0), -1, b">= 1"), (dict(mem_size=33), -4, b"mem_size"),
    (dict(agent_dim=33), -4, b"agent_dim"), (dict(n_features=1003), -4, b"1024"), (dict(h1=48), -4, b"multiples of 32"),
    (dict(h3=512), -4, b"multiples of 32"), (dict(n_rot=33), -4, b"n_rot"),
])
def test_tiles_forward_shape_validation(lib, kw, code, msg):
    assert forward(lib, shape(**kw)) == code, kw
    assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    assert forward(lib, None) == -1 and b"NULL shape" in lib.antsrl_last_error()


# ---- the restatement's own properties
SWEEP = [(4, 64, 0.5, 0, 0), (7, 33, 0.3, 5, 0), (16, 512, 0.5, 123456789, 0), (5, 17, 0.5, 2, 3), (3, 1, 0.5, 9, 1 << 20),
         (64, 64, 0.1, 4, 0), (6, 50, 0.5, 3, 0), (9, 50, 0.9, 1, 7)]


@pytest.mark.parametrize("E,N,eps,step,base", SWEEP)
def test_epsilon_0_lists_every_tile_and_epsilon_1_none(E, N, eps, step, base):
    T = P.n_tiles(E, N)
    assert np.array_equal(P.live_tiles(11, step, base, E, N, 0.0), np.arange(T))
    assert P.live_tiles(11, step, base, E, N, 1.0).size == 0


@pytest.mark.parametrize("E,N,eps,step,base", SWEEP)
def test_listed_tiles_are_exactly_those_with_an_ant_that_acts(E, N, eps, step, base):
    """Written the slow way, ant by ant, against the restatement's reshape."""
    seed = 1234567 + E
    ex = R.explores(seed, step, base, E, eps)
    want = sorted({i // 32 for i in range(E * N) if not ex[i // N]})
    got = P.live_tiles(seed, step, base, E, N, eps)
    assert got.dtype == np.int32 and got.tolist() == want
    assert np.all(np.diff(got) > 0) and (got.size == 0 or (got[0] >= 0 and got[-1] < P.n_tiles(E, N)))


def test_a_tile_that_straddles_an_exploring_and_an_acting_environment_is_live():
    """n_ants = 50: tile 1 = ants 32..63 holds ants of environments 0 and 1."""
    E, N, eps, found = 8, 50, 0.5, 0
    for seed in range(40):
        ex = R.explores(seed, 0, 0, E, eps)
        live = set(P.live_tiles(seed, 0, 0, E, N, eps).tolist())
        for t in range(P.n_tiles(E, N)):
            envs = sorted({i // N for i in range(32 * t, min(32 * t + 32, E * N))})
            if len(envs) == 2 and ex[envs[0]] != ex[envs[1]]:
                assert t in live
                found += 1
            if all(ex[e] for e in envs):
                assert t not in live
    assert found > 20
