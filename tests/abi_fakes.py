"""What the CPU-side checks of the C-ABI entries share (the *_abi_cpu.py files and their helpers): the library, the
return codes and fake device pointers.  The pointers are never dereferenced: every call made with them fails validation
(or is host arithmetic).  A test module imports `lib` to get the fixture."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -4  # include/antsrl.h ANTSRL_E_INVALID, ANTSRL_E_UNSUPPORTED

FAKE = C.c_void_p(1 << 20)  # 256-byte aligned
ODD = C.c_void_p((1 << 20) + 2)  # 2-byte aligned only
ODD4 = C.c_void_p((1 << 20) + 4)
ODD8 = C.c_void_p((1 << 20) + 8)
ODD128 = C.c_void_p((1 << 20) + 128)


@pytest.fixture(scope="module")
def lib():
    from antsrl_amd import _lib
    from antsrl_amd import build as buildmod
    buildmod.build_hip()
    return _lib.load()
