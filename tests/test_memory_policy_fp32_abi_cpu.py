"""CPU-side checks of the memory agent net's precision-aware C-ABI entries (antsrl_memnet_packed_bytes_ex,
antsrl_memnet_pack_ex, antsrl_policy_memory_ex): exported, the fp32 packed size is the documented formula, the bf16
precision is the old entries' size, and every validation rule (an unknown precision included) refuses before any HIP
call.  No kernel is launched here: every call below fails validation, and the pointers are fakes never dereferenced."""
import ctypes as C

import pytest

from abi_fakes import FAKE, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_memnet_packed_bytes_ex", "antsrl_memnet_pack_ex", "antsrl_policy_memory_ex")
BF16, FP32 = 0, 1


def shape(F=294, power=5, mem=20, n_rot=3, n_ph=3, agent_dim=2):
    return _lib.AntsMemNetShape(F, agent_dim, mem, 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power), n_rot, n_ph)


def documented_fp32_bytes(F, power, mem):
    """include/antsrl.h: sum over the twelve packed layers of round256(1024 (in/8)(out/32)) + round256(4 out)."""
    D = F + 2 + mem
    Dp = (D + 31) // 32 * 32
    h1, h2, h3 = 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power)
    r = lambda v: (v + 255) // 256 * 256  # noqa: E731
    layers = [(Dp, h2), (h2, h3), (h3, h1), (h1, Dp), (Dp, h2), (h2, h3), (h3, 32), (Dp, h1), (h1, 32), (Dp, h2), (h2, h2),
              (h2, 64)]
    return sum(r(1024 * (i // 8) * (o // 32)) + r(4 * o) for i, o in layers)


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS


@pytest.mark.parametrize("power,mem,want", [(5, 20, 1128960), (4, 10, 467456)])
def test_fp32_packed_bytes_is_the_documented_size(lib, power, mem, want):
    n = C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes_ex(C.byref(shape(power=power, mem=mem)), FP32, C.byref(n)) == 0
    assert n.value == documented_fp32_bytes(294, power, mem) == want


@pytest.mark.parametrize("F,power,mem", [(294, 5, 20), (294, 4, 10), (296, 5, 2), (298, 4, 20), (299, 5, 20),
                                         (990, 5, 32), (294, 4, 1), (1, 4, 1), (700, 4, 7)])
def test_sizes_across_shapes(lib, F, power, mem):
    """fp32: the formula, D = 321 and D = 1024 included; bf16 through _ex: exactly the old entry's size."""
    s = shape(F=F, power=power, mem=mem)
    n32, n16, old = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes_ex(C.byref(s), FP32, C.byref(n32)) == 0
    assert lib.antsrl_memnet_packed_bytes_ex(C.byref(s), BF16, C.byref(n16)) == 0
    assert lib.antsrl_memnet_packed_bytes(C.byref(s), C.byref(old)) == 0
    assert n32.value == documented_fp32_bytes(F, power, mem)
    assert n16.value == old.value
    assert old.value < n32.value <= 2 * old.value  # 4 bytes per weight instead of 2, the same biases


# (FAKE is never dereferenced: every call below fails validation first)
def policy(lib, s, precision=FP32, packed=FAKE, obs=FAKE, rot=FAKE, n_ants=64, fmt=0):
    return lib.antsrl_policy_memory_ex(C.byref(s) if s is not None else None, precision, packed, obs, fmt, FAKE, FAKE,
                                       n_ants, FAKE, rot, None, None, None)


def old_policy(lib, s, packed=FAKE, obs=FAKE, rot=FAKE, n_ants=64, fmt=0):
    return lib.antsrl_policy_memory(C.byref(s) if s is not None else None, packed, obs, fmt, FAKE, FAKE, n_ants, FAKE, rot,
                                    None, None, None)


@pytest.mark.parametrize("precision", [-1, 2, 7, 1 << 30])
def test_unknown_precision_is_refused(lib, precision):
    s = shape()
    n = C.c_size_t()
    want = b"precision %d" % precision
    assert lib.antsrl_memnet_packed_bytes_ex(C.byref(s), precision, C.byref(n)) == -1
    assert want in lib.antsrl_last_error()
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 26))
    assert lib.antsrl_memnet_pack_ex(C.byref(s), precision, ptrs, FAKE, None) == -1
    assert want in lib.antsrl_last_error()
    assert policy(lib, s, precision=precision) == -1
    assert want in lib.antsrl_last_error()
    assert policy(lib, None, precision=precision) == -1 and want in lib.antsrl_last_error()  # checked first


@pytest.mark.parametrize("precision", [BF16, FP32])
@pytest.mark.parametrize("kw,code,msg", [
    (dict(F=1023), -4, b"1024"),                 # D = 1023 + 2 + 20 > 1024
    (dict(power=6), -4, b"256"),                 # h3 = 512
    (dict(mem=0), -1, b">= 1"),
    (dict(mem=33), -4, b"mem_size"),
    (dict(n_rot=33), -4, b"n_rot"),
    (dict(n_ph=0), -1, b">= 1"),
    (dict(agent_dim=33), -4, b"agent_dim"),
])
def test_shape_validation_matches_the_bf16_entries(lib, precision, kw, code, msg):
    s = shape(**kw)
    n = C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes(C.byref(s), C.byref(n)) == code
    assert lib.antsrl_memnet_packed_bytes_ex(C.byref(s), precision, C.byref(n)) == code
    assert msg in lib.antsrl_last_error()
    assert old_policy(lib, s) == code
    assert policy(lib, s, precision=precision) == code
    assert msg in lib.antsrl_last_error()
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 26))
    assert lib.antsrl_memnet_pack(C.byref(s), ptrs, FAKE, None) == code
    assert lib.antsrl_memnet_pack_ex(C.byref(s), precision, ptrs, FAKE, None) == code


@pytest.mark.parametrize("precision", [BF16, FP32])
def test_pointer_and_count_validation_matches_the_bf16_entries(lib, precision):
    s = shape()
    for kw, msg in ((dict(packed=None), b"packed"), (dict(obs=None), b"obs"), (dict(rot=None), b"rotation"),
                    (dict(n_ants=0), b"n_ants"), (dict(n_ants=-5), b"n_ants"), (dict(n_ants=1 << 31), b"n_ants"),
                    (dict(fmt=2), b"obs_format"), (dict(packed=C.c_void_p((1 << 20) + 16)), b"aligned")):
        assert old_policy(lib, s, **kw) == -1, kw
        assert policy(lib, s, precision=precision, **kw) == -1, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    assert policy(lib, None, precision=precision) == -1 and b"NULL shape" in lib.antsrl_last_error()
    n = C.c_size_t()
    assert lib.antsrl_memnet_packed_bytes_ex(C.byref(s), precision, None) == -1
    assert lib.antsrl_memnet_pack_ex(C.byref(s), precision, None, FAKE, None) == -1 and b"params" in lib.antsrl_last_error()
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 26))
    assert lib.antsrl_memnet_pack_ex(C.byref(s), precision, ptrs, None, None) == -1
    assert lib.antsrl_memnet_pack_ex(C.byref(s), precision, ptrs, C.c_void_p((1 << 20) + 64), None) == -1
    assert b"aligned" in lib.antsrl_last_error()
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 25 + [0]))
    assert lib.antsrl_memnet_pack_ex(C.byref(s), precision, ptrs, FAKE, None) == -1
    assert b"params[25]" in lib.antsrl_last_error()
    assert lib.antsrl_memnet_packed_bytes_ex(C.byref(s), precision, C.byref(n)) == 0  # the valid shape itself is fine


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_policy_on_cpu_holds_weights_only(lib, precision):
    import torch
    from antsrl_amd.policy import MemoryPolicy
    pol = MemoryPolicy(294, "cpu", power=4, mem_size=10, seed=3, precision=precision)
    assert pol.precision == precision and pol.packed is None
    ref = MemoryPolicy(294, "cpu", power=4, mem_size=10, seed=3)
    assert ref.precision == "bf16"
    sd = pol.state_dict()
    assert set(sd) == set(ref.state_dict()) and all(torch.equal(sd[k], ref.state_dict()[k]) for k in sd)
    pol.load_state_dict({k: v * 2 for k, v in sd.items()})
    assert pol.precision == precision and pol.packed is None
    with pytest.raises(AssertionError):
        pol.act(torch.zeros((1, 7, 7, 6)), torch.zeros((1, 2)))


def test_unknown_precision_name_is_refused(lib):
    from antsrl_amd.policy import MemoryPolicy
    with pytest.raises(AssertionError, match="precision"):
        MemoryPolicy(294, "cpu", precision="fp16")
