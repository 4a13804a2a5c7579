"""CPU-side checks of the memory agent net's C-ABI entries (antsrl_memnet_packed_bytes, antsrl_memnet_pack,
antsrl_policy_memory): exported, the packed size is the documented formula, and every validation rule refuses with a
message before any HIP call.  No kernel is launched here: every call below fails validation, and the pointers are
fakes that are never dereferenced."""
import ctypes as C

import pytest

from abi_fakes import FAKE, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_memnet_packed_bytes", "antsrl_memnet_pack", "antsrl_policy_memory")


def shape(F=294, power=5, mem=20, n_rot=3, n_ph=3, agent_dim=2):
    return _lib.AntsMemNetShape(F, agent_dim, mem, 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power), n_rot, n_ph)


def documented_bytes(F, power, mem):
    """include/antsrl.h: sum over the twelve packed layers of round256(1024 (in/16)(out/32)) + round256(4 out)."""
    D = F + 2 + mem
    Dp = (D + 31) // 32 * 32
    h1, h2, h3 = 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power)
    r = lambda v: (v + 255) // 256 * 256  # noqa: E731
    layers = [(Dp, h2), (h2, h3), (h3, h1), (h1, Dp), (Dp, h2), (h2, h3), (h3, 32), (Dp, h1), (h1, 32), (Dp, h2), (h2, h2),
              (h2, 64)]
    return sum(r(1024 * (i // 16) * (o // 32)) + r(4 * o) for i, o in layers)


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS


@pytest.mark.parametrize("power,mem,want", [(5, 20, 567808), (4, 10, 236032)])
def test_packed_bytes_is_the_documented_size(lib, power, mem, want):
    n = C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes(C.byref(shape(power=power, mem=mem)), C.byref(n)) == 0
    assert n.value == documented_bytes(294, power, mem) == want
    # the bf16 weights themselves: ~535 KiB at power 5, ~210 KiB at power 4, plus padding to whole fragments
    assert 0.9 * want < n.value <= want


# (FAKE is never dereferenced: every call below fails validation first)
def policy(lib, s, packed=FAKE, obs=FAKE, rot=FAKE, n_ants=64, fmt=0):
    return lib.antsrl_policy_memory(C.byref(s) if s is not None else None, packed, obs, fmt, FAKE, FAKE, n_ants, FAKE, rot,
                                    None, None, None)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(F=1023), -4, b"1024"),                 # D = 1023 + 2 + 20 > 1024
    (dict(power=6), -4, b"256"),                 # h3 = 512
    (dict(mem=0), -1, b">= 1"),
    (dict(mem=33), -4, b"mem_size"),
    (dict(n_rot=33), -4, b"n_rot"),
    (dict(n_ph=0), -1, b">= 1"),
])
def test_shape_validation(lib, kw, code, msg):
    s = shape(**kw)
    n = C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes(C.byref(s), C.byref(n)) == code
    assert msg in lib.antsrl_last_error()
    assert policy(lib, s) == code
    assert msg in lib.antsrl_last_error()
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 26))
    assert lib.antsrl_memnet_pack(C.byref(s), ptrs, FAKE, None) == code


def test_h_must_be_multiples_of_32(lib):
    s = shape()
    s.h2 = 100
    assert policy(lib, s) == -4 and b"multiples of 32" in lib.antsrl_last_error()


def test_pointer_and_count_validation(lib):
    s = shape()
    for kw, msg in ((dict(packed=None), b"packed"), (dict(obs=None), b"obs"), (dict(rot=None), b"rotation"),
                    (dict(n_ants=0), b"n_ants"), (dict(n_ants=-5), b"n_ants"), (dict(fmt=2), b"obs_format"),
                    (dict(packed=C.c_void_p((1 << 20) + 16)), b"aligned")):
        assert policy(lib, s, **kw) == -1, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    assert policy(lib, None) == -1 and b"NULL shape" in lib.antsrl_last_error()
    n = C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes(C.byref(s), None) == -1
    assert lib.antsrl_memnet_pack(C.byref(s), None, FAKE, None) == -1 and b"params" in lib.antsrl_last_error()
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 25 + [0]))
    assert lib.antsrl_memnet_pack(C.byref(s), ptrs, FAKE, None) == -1 and b"params[25]" in lib.antsrl_last_error()
    assert lib.antsrl_memnet_packed_bytes(C.byref(s), C.byref(n)) == 0  # the valid shape itself is fine


def test_shape_helpers():
    from antsrl_amd.policy import memnet_param_shapes, memnet_shape_from_state_dict
    import torch
    for power, mem in ((4, 10), (5, 20)):
        sd = {}
        for name, (o, i) in memnet_param_shapes(294, power, mem, 3, 4).items():
            sd[name + ".weight"], sd[name + ".bias"] = torch.zeros(o, i), torch.zeros(o)
        assert memnet_shape_from_state_dict(sd) == dict(power=power, mem_size=mem, n_rot=3, n_ph=4, n_features=294)
