"""CPU-side checks of the rework agent's fused act + select entry (antsrl_policy_rework_select) and of ReworkAgent's
construction: the symbol is exported and declared, and every validation rule refuses with its code and a message before
any HIP call.  No kernel is launched here: every call below fails validation, and the pointers are fakes that are never
dereferenced."""
import ctypes as C
import os

import pytest

from abi_fakes import FAKE, INVALID, ODD, UNSUPPORTED, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NAME = "antsrl_policy_rework_select"
FIELDS = ("n_features", "agent_dim", "g1", "g2", "g3", "r1", "r2", "r3", "p1", "n_rot", "n_ph")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "antsrl.h")


def shape(**kw):
    v = dict(n_features=294, agent_dim=2, g1=64, g2=128, g3=32, r1=64, r2=128, r3=32, p1=32, n_rot=3, n_ph=3)
    v.update(kw)
    return _lib.AntsReworkShape(*[v[n] for n in FIELDS])


def select(lib, s, collapsed=FAKE, obs=FAKE, fmt=0, ast=FAKE, seed=1, step=2, base=0, n_envs=4, n_ants=64, epsilon=0.5,
           rot=FAKE, ph=FAKE, explored=FAKE, q=None):
    return lib.antsrl_policy_rework_select(C.byref(s) if s is not None else None, collapsed, obs, fmt, ast, seed, step, base,
                                           n_envs, n_ants, epsilon, rot, ph, explored, q, None)


def test_the_symbol_is_exported_and_declared(lib):
    assert hasattr(lib, NAME) and NAME in _lib.EXPORTS
    text = open(HEADER).read()
    assert "int %s(const AntsReworkShape *s" % NAME in text
    assert "#define ANTSRL_ABI_VERSION 5" in text and lib.antsrl_abi_version() == 5  # an additive entry


def test_pointer_and_format_validation(lib):
    s = shape()
    for kw, msg in ((dict(collapsed=None), b"collapsed"), (dict(obs=None), b"obs"), (dict(ast=None), b"agent_state"),
                    (dict(rot=None), b"rotation"), (dict(ph=None), b"pheromone"), (dict(collapsed=ODD), b"aligned"),
                    (dict(obs=ODD), b"aligned"), (dict(ast=ODD), b"aligned"), (dict(q=ODD), b"aligned"),
                    (dict(fmt=2), b"obs_format"), (dict(fmt=-1), b"obs_format")):
        assert select(lib, s, **kw) == INVALID, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    assert select(lib, None) == INVALID and b"NULL shape" in lib.antsrl_last_error()


@pytest.mark.parametrize("epsilon", [-1e-9, 1.0000001, 2.0, -1.0, float("nan"), float("inf")])
def test_epsilon_outside_the_unit_interval(lib, epsilon):
    assert select(lib, shape(), epsilon=epsilon) == INVALID
    assert b"epsilon" in lib.antsrl_last_error()


@pytest.mark.parametrize("kw,msg", [
    (dict(n_envs=0), b">= 1"), (dict(n_ants=0), b">= 1"), (dict(n_envs=-3), b">= 1"), (dict(n_ants=-1), b">= 1"),
    (dict(n_envs=1 << 16, n_ants=1 << 15), b"2^31"),          # n_envs * n_ants == 2^31
    (dict(n_envs=46341, n_ants=46341), b"2^31"),              # just above
    (dict(base=-1), b"env_id_base"),
    (dict(base=(1 << 31) - 4, n_envs=4), b"env_id_base"),     # env_id_base + n_envs == 2^31
    (dict(base=(1 << 31) - 1, n_envs=1, n_ants=1), b"env_id_base"),
])
def test_batch_validation(lib, kw, msg):
    assert select(lib, shape(), **kw) == INVALID, kw
    assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())


@pytest.mark.parametrize("kw,code,msg", [
    (dict(n_features=1023), UNSUPPORTED, b"1024"),
    (dict(agent_dim=3), UNSUPPORTED, b"agent_dim"),
    (dict(g2=257), UNSUPPORTED, b"g2"),
    (dict(n_rot=9), UNSUPPORTED, b"n_rot"),
    (dict(n_ph=9), UNSUPPORTED, b"n_ph"),
    (dict(n_features=0), INVALID, b">= 1"),
    (dict(n_rot=0), INVALID, b">= 1"),
    (dict(p1=0), INVALID, b"p1"),
])
def test_shape_validation(lib, kw, code, msg):
    assert select(lib, shape(**kw)) == code
    assert msg in lib.antsrl_last_error()


def test_the_shape_is_checked_first_and_the_batch_last(lib):
    """One failing argument at a time is covered above; with several, the order is the shape, the pointers, the format,
    the batch, epsilon."""
    assert select(lib, shape(n_rot=9), obs=None, n_envs=0, epsilon=2.0) == UNSUPPORTED
    assert select(lib, shape(), obs=None, n_envs=0, epsilon=2.0) == INVALID and b"obs" in lib.antsrl_last_error()
    assert select(lib, shape(), fmt=7, n_envs=0, epsilon=2.0) == INVALID and b"obs_format" in lib.antsrl_last_error()
    assert select(lib, shape(), n_envs=0, epsilon=2.0) == INVALID and b">= 1" in lib.antsrl_last_error()


def test_rework_agent_is_importable_and_checks_its_heads():
    import antsrl_amd
    from antsrl_amd.agent import ReworkAgent, _DeviceAgent
    assert antsrl_amd.ReworkAgent is ReworkAgent and "ReworkAgent" in antsrl_amd.__all__
    assert issubclass(ReworkAgent, _DeviceAgent)
    a = ReworkAgent()
    assert a.name == "collect_agent_rework" and a.fused_select is True
    assert (a.epsilon, a.discount, a.rotations, a.pheromones, a.learning_rate) == (0.1, 0.5, 3, 3, 1e-4)
    assert (a.record_per_step, a.replay_size, a.minibatch, a.min_replay, a.update_target_every, a.seed) == (None, 50000, 264,
                                                                                                           1000, 1, 0)
    a.epsilon = 0.3  # settable, as the reference's main loop sets it every episode
    assert a.epsilon == 0.3
    for r, p in ((1, 8), (8, 1), (2, 5)):
        b = ReworkAgent(rotations=r, pheromones=p, fused_select=False)
        assert (b.rotations, b.pheromones, b.fused_select) == (r, p, False)
    for r, p in ((0, 3), (9, 3), (3, 0), (3, 9), (-1, 3)):
        with pytest.raises(AssertionError, match="1 to 8"):
            ReworkAgent(rotations=r, pheromones=p)
