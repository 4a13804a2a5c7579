"""CPU-side checks of the rework agent net's C-ABI entries (antsrl_rework_collapsed_bytes, antsrl_rework_collapse,
antsrl_policy_rework): exported, the collapsed size is the documented formula, and every validation rule refuses with its
code and a message before any HIP call.  No kernel is launched here: every call below fails validation or has nothing
to launch, and the pointers are fakes that are never dereferenced."""
import ctypes as C

import pytest

from abi_fakes import FAKE, INVALID, UNSUPPORTED, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_rework_collapsed_bytes", "antsrl_rework_collapse", "antsrl_policy_rework")
FIELDS = ("n_features", "agent_dim", "g1", "g2", "g3", "r1", "r2", "r3", "p1", "n_rot", "n_ph")


def shape(**kw):
    v = dict(n_features=294, agent_dim=2, g1=64, g2=128, g3=32, r1=64, r2=128, r3=32, p1=32, n_rot=3, n_ph=3)
    v.update(kw)
    return _lib.AntsReworkShape(*[v[n] for n in FIELDS])


def fake_params(n_null=None, misaligned=None):
    p = [FAKE.value] * 20
    if n_null is not None:
        p[n_null] = 0
    if misaligned is not None:
        p[misaligned] += 2
    return (C.c_void_p * 20)(*p)


def policy(lib, s, collapsed=FAKE, obs=FAKE, ast=FAKE, rot=FAKE, ph=FAKE, q=None, n_ants=64, fmt=0):
    return lib.antsrl_policy_rework(C.byref(s) if s is not None else None, collapsed, obs, fmt, ast, n_ants, rot, ph, q, None)


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS
    assert [f for f, _ in _lib.AntsReworkShape._fields_] == list(FIELDS) and C.sizeof(_lib.AntsReworkShape) == 44


@pytest.mark.parametrize("kw,want", [(dict(), 7128), (dict(n_features=1022, n_rot=8, n_ph=8), 4 * (16 * 1024 + 16)),
                                      (dict(n_features=1, n_rot=1, n_ph=1), 4 * (2 * 3 + 2)),
                                      (dict(n_features=147, n_rot=5, n_ph=2, g1=1, p1=256), 4 * (7 * 149 + 7))])
def test_collapsed_bytes_is_the_documented_size(lib, kw, want):
    """include/antsrl.h: 4 * (NQ * D + NQ) with NQ = n_rot + n_ph, D = n_features + 2."""
    s = shape(**kw)
    n = C.c_size_t()
    assert lib.antsrl_rework_collapsed_bytes(C.byref(s), C.byref(n)) == 0
    assert n.value == 4 * ((s.n_rot + s.n_ph) * (s.n_features + 2) + s.n_rot + s.n_ph) == want


@pytest.mark.parametrize("kw,code,msg", [
    (dict(n_features=1023), UNSUPPORTED, b"1024"),   # D = 1025
    (dict(agent_dim=3), UNSUPPORTED, b"agent_dim"),
    (dict(agent_dim=1), UNSUPPORTED, b"agent_dim"),
    (dict(g2=257), UNSUPPORTED, b"g2"),
    (dict(r3=512), UNSUPPORTED, b"r3"),
    (dict(p1=300), UNSUPPORTED, b"p1"),
    (dict(n_rot=9), UNSUPPORTED, b"n_rot"),
    (dict(n_ph=9), UNSUPPORTED, b"n_ph"),
    (dict(n_features=0), INVALID, b">= 1"),
    (dict(agent_dim=0), INVALID, b">= 1"),
    (dict(g1=0), INVALID, b"g1"),
    (dict(r2=-4), INVALID, b"r2"),
    (dict(p1=0), INVALID, b"p1"),
    (dict(n_rot=0), INVALID, b">= 1"),
    (dict(n_ph=-1), INVALID, b">= 1"),
    (dict(n_ph=0, n_features=5000), INVALID, b">= 1"),  # a value < 1 is invalid whatever else is out of range
])
def test_shape_validation(lib, kw, code, msg):
    s = shape(**kw)
    n = C.c_size_t()
    assert lib.antsrl_rework_collapsed_bytes(C.byref(s), C.byref(n)) == code
    assert msg in lib.antsrl_last_error()
    assert policy(lib, s) == code
    assert msg in lib.antsrl_last_error()
    assert lib.antsrl_rework_collapse(C.byref(s), fake_params(), FAKE, None) == code
    assert msg in lib.antsrl_last_error()


def test_every_limit_itself_is_supported(lib):
    n = C.c_size_t()
    s = shape(n_features=1022, g1=256, g2=256, g3=256, r1=256, r2=256, r3=256, p1=256, n_rot=8, n_ph=8)
    assert lib.antsrl_rework_collapsed_bytes(C.byref(s), C.byref(n)) == 0
    s = shape(n_features=1, g1=1, g2=1, g3=1, r1=1, r2=1, r3=1, p1=1, n_rot=1, n_ph=1)
    assert lib.antsrl_rework_collapsed_bytes(C.byref(s), C.byref(n)) == 0


def test_pointer_format_and_count_validation(lib):
    s = shape()
    odd = C.c_void_p((1 << 20) + 2)
    for kw, msg in ((dict(collapsed=None), b"collapsed"), (dict(obs=None), b"obs"), (dict(ast=None), b"agent_state"),
                    (dict(rot=None), b"rotation"), (dict(ph=None), b"pheromone"), (dict(n_ants=-1), b"n_ants"),
                    (dict(n_ants=1 << 31), b"n_ants"), (dict(fmt=2), b"obs_format"), (dict(fmt=-1), b"obs_format"),
                    (dict(collapsed=odd), b"aligned"), (dict(obs=odd), b"aligned"), (dict(ast=odd), b"aligned"),
                    (dict(q=odd), b"aligned")):
        assert policy(lib, s, **kw) == INVALID, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    assert policy(lib, None) == INVALID and b"NULL shape" in lib.antsrl_last_error()
    assert lib.antsrl_rework_collapsed_bytes(None, C.byref(C.c_size_t())) == INVALID
    assert lib.antsrl_rework_collapsed_bytes(C.byref(s), None) == INVALID and b"bytes" in lib.antsrl_last_error()
    assert lib.antsrl_rework_collapse(C.byref(s), None, FAKE, None) == INVALID and b"params" in lib.antsrl_last_error()
    assert lib.antsrl_rework_collapse(C.byref(s), fake_params(), None, None) == INVALID and b"collapsed" in lib.antsrl_last_error()
    assert lib.antsrl_rework_collapse(C.byref(s), fake_params(), odd, None) == INVALID and b"aligned" in lib.antsrl_last_error()
    assert lib.antsrl_rework_collapse(C.byref(s), fake_params(n_null=19), FAKE, None) == INVALID
    assert b"params[19]" in lib.antsrl_last_error()
    assert lib.antsrl_rework_collapse(C.byref(s), fake_params(misaligned=7), FAKE, None) == INVALID
    assert b"params[7]" in lib.antsrl_last_error()


def test_no_ants_succeed_and_launch_nothing(lib):
    """n_ants == 0 returns before any HIP call: it succeeds here, where there is no device to launch on."""
    assert policy(lib, shape(), n_ants=0) == 0
    assert policy(lib, shape(), n_ants=0, fmt=1) == 0
    assert policy(lib, shape(), n_ants=0, fmt=3) == INVALID  # ... but only behind every check


def test_weights_only_policy_on_the_cpu(lib):
    """ReworkPolicy without a device holds and reloads weights under the reference's names; act needs a GPU."""
    import torch
    from antsrl_amd.policy import REWORK_LAYERS, ReworkPolicy, rework_param_shapes
    p = ReworkPolicy(147, "cpu", n_rot=5, n_ph=2, seed=3)
    sd = p.state_dict()
    assert list(sd) == [l + s for l in REWORK_LAYERS for s in (".weight", ".bias")]
    for l, (o, i) in rework_param_shapes(147, 5, 2).items():
        assert tuple(sd[l + ".weight"].shape) == (o, i) and tuple(sd[l + ".bias"].shape) == (o,)
        assert sd[l + ".weight"].dtype == torch.float32 and float(sd[l + ".weight"].abs().max()) <= 1 / i ** 0.5
    q = ReworkPolicy(147, "cpu", n_rot=3, n_ph=3, seed=4)
    q.load_state_dict(sd)
    assert (q.n_rot, q.n_ph) == (5, 2) and all(torch.equal(q.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(AssertionError, match="features"):
        ReworkPolicy(294, "cpu").load_state_dict(sd)
    with pytest.raises(AssertionError, match="GPU"):
        p.act(torch.zeros(1, 7, 7, 3), torch.zeros(1, 2))
