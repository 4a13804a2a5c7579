"""CPU-side checks of the training step's C-ABI entries (antsrl_memtrain_*): exported, the sizes are the documented
formulas, and every invalid shape or pointer is refused with a message before any HIP call.  No kernel is launched
here: every call below fails validation, and the pointers are fakes that are never dereferenced."""
import ctypes as C

import pytest

from abi_fakes import FAKE, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

NEW = ("antsrl_memtrain_sizes", "antsrl_memtrain_init", "antsrl_memtrain_unpack", "antsrl_memtrain_copy",
       "antsrl_memtrain_grad", "antsrl_memtrain_apply")


def shape(F=294, power=5, mem=20, n_rot=3, n_ph=3, agent_dim=2):
    return _lib.AntsMemNetShape(F, agent_dim, mem, 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power), n_rot, n_ph)


def documented(F, power, mem, n_rot=3, n_ph=3, B=264):
    """include/antsrl.h, antsrl_memtrain_sizes."""
    D = F + 2 + mem
    h1, h2, h3 = 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power)
    layers = [(h2, D), (h3, h2), (h1, h3), (D, h1), (h2, D), (h3, h2), (n_rot, h3), (h1, D), (n_ph, h1),
              (h2, D), (h2, h2), (mem, h2), (mem, h2)]
    params = sum(o * i + o for o, i in layers)
    trained = sum(o * i + o for o, i in layers[:9])
    r = lambda v, a: (v + a - 1) // a * a  # noqa: E731
    packs = sum(2 * r(o, 32) * r(i, 32) for o, i in layers[:9])
    m_off = r(4 * params, 256)
    v_off = r(m_off + 4 * trained, 256)
    state = r(r(v_off + 4 * trained, 256) + 2 * packs, 256)
    Bp = r(B, 32)
    nch = min(64, (Bp + 255) // 256)
    chunk = r((Bp + nch - 1) // nch, 32)
    nch = (Bp + chunk - 1) // chunk
    widths = [r(o, 32) for o, _ in layers[:9]]
    floats = [3 * Bp * w for w in widths]  # target and model outputs, the model's output gradients
    floats.append(nch * sum(r(o, 32) * r(i, 32) + r(o, 32) for o, i in layers[:9]))
    floats.append((Bp + 255) // 256)
    work = 4 * sum(r(f, 64) for f in floats)
    return params, trained, state, work


def sizes(lib, s, B=264):
    out = [C.c_size_t() for _ in range(4)]
    rc = lib.antsrl_memtrain_sizes(C.byref(s) if s is not None else None, B, *[C.byref(o) for o in out])
    return rc, [o.value for o in out]


def test_new_symbols_are_exported(lib):
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS


@pytest.mark.parametrize("power,mem", [(5, 20), (4, 10)])
@pytest.mark.parametrize("B", [1, 33, 264, 4097, 65536])
def test_sizes_are_the_documented_formulas(lib, power, mem, B):
    rc, got = sizes(lib, shape(power=power, mem=mem), B)
    assert rc == 0
    assert got == list(documented(294, power, mem, B=B))


def test_power5_counts():
    params, trained, _, _ = documented(294, 5, 20)
    assert (trained, params) == (205_442, 267_690)
    assert params - trained == (128 * 316 + 128) + (128 * 128 + 128) + 2 * (20 * 128 + 20)


@pytest.mark.parametrize("kw,code,msg", [
    (dict(F=1023), -4, b"1024"),
    (dict(power=6), -4, b"256"),
    (dict(mem=0), -1, b">= 1"),
    (dict(mem=33), -4, b"mem_size"),
    (dict(n_rot=33), -4, b"n_rot"),
    (dict(n_ph=0), -1, b">= 1"),
])
def test_shape_validation(lib, kw, code, msg):
    s = shape(**kw)
    assert sizes(lib, s)[0] == code and msg in lib.antsrl_last_error()
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 26))
    assert lib.antsrl_memtrain_init(C.byref(s), ptrs, FAKE, None) == code and msg in lib.antsrl_last_error()
    assert lib.antsrl_memtrain_unpack(C.byref(s), FAKE, ptrs, None) == code
    assert lib.antsrl_memtrain_copy(C.byref(s), FAKE, FAKE, None) == code
    assert grad(lib, s) == code and msg in lib.antsrl_last_error()
    assert lib.antsrl_memtrain_apply(C.byref(s), FAKE, FAKE, 1, 1e-4, 0.9, 0.999, 1e-8, None) == code


def grad(lib, s, B=264, **kw):
    a = dict(state=FAKE, target=FAKE, states=FAKE, agent_states=FAKE, actions=FAKE, rewards=FAKE, new_states=FAKE,
             new_agent_states=FAKE, dones=FAKE, idx=None, grads=FAKE, loss=FAKE, work=FAKE, discount=0.99)
    a.update(kw)
    return lib.antsrl_memtrain_grad(C.byref(s) if s is not None else None, a["state"], a["target"], a["states"],
                                    a["agent_states"], a["actions"], a["rewards"], a["new_states"], a["new_agent_states"],
                                    a["dones"], a["idx"], B, a["discount"], a["grads"], a["loss"], a["work"], None)


def test_pointer_and_count_validation(lib):
    s = shape()
    assert grad(lib, None) == -1 and b"NULL shape" in lib.antsrl_last_error()
    for kw, msg in ((dict(state=None), b"state"), (dict(target=None), b"target_state"), (dict(work=None), b"workspace"),
                    (dict(state=C.c_void_p((1 << 20) + 16)), b"aligned"), (dict(states=None), b"states"),
                    (dict(dones=None), b"dones"), (dict(actions=None), b"actions"), (dict(grads=None), b"grads"),
                    (dict(loss=None), b"loss_out"), (dict(idx=C.c_void_p((1 << 20) + 4)), b"8-byte"),
                    (dict(rewards=C.c_void_p((1 << 20) + 2)), b"4-byte"), (dict(discount=float("nan")), b"NaN")):
        assert grad(lib, s, **kw) == -1, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    for B in (0, -3, (1 << 24) + 1):
        assert grad(lib, s, B=B) == -1 and b"B must be" in lib.antsrl_last_error()
        assert sizes(lib, s, B)[0] == -1
    ap = lambda **kw: lib.antsrl_memtrain_apply(C.byref(s), kw.get("state", FAKE), kw.get("grads", FAKE),  # noqa: E731
                                                kw.get("step", 1), kw.get("lr", 1e-4), kw.get("b1", 0.9),
                                                kw.get("b2", 0.999), kw.get("eps", 1e-8), None)
    for kw, msg in ((dict(state=None), b"state"), (dict(grads=None), b"grads"), (dict(step=0), b"step"),
                    (dict(lr=-1.0), b"lr"), (dict(lr=float("nan")), b"lr"), (dict(b1=1.0), b"beta"),
                    (dict(b2=-0.1), b"beta"), (dict(eps=0.0), b"eps")):
        assert ap(**kw) == -1, kw
        assert msg in lib.antsrl_last_error(), (kw, lib.antsrl_last_error())
    ptrs = (C.c_void_p * 26)(*([FAKE.value] * 25 + [0]))
    assert lib.antsrl_memtrain_init(C.byref(s), ptrs, FAKE, None) == -1 and b"params[25]" in lib.antsrl_last_error()
    assert lib.antsrl_memtrain_init(C.byref(s), None, FAKE, None) == -1 and b"params" in lib.antsrl_last_error()
    ok = (C.c_void_p * 26)(*([FAKE.value] * 26))
    assert lib.antsrl_memtrain_init(C.byref(s), ok, None, None) == -1 and b"state" in lib.antsrl_last_error()
    assert lib.antsrl_memtrain_unpack(C.byref(s), FAKE, ptrs, None) == -1 and b"params[25]" in lib.antsrl_last_error()
    assert lib.antsrl_memtrain_copy(C.byref(s), None, FAKE, None) == -1 and b"src_state" in lib.antsrl_last_error()
    assert lib.antsrl_memtrain_copy(C.byref(s), FAKE, C.c_void_p((1 << 20) + 8), None) == -1
    assert b"dst_state" in lib.antsrl_last_error()
    assert sizes(lib, s)[0] == 0  # the valid shape itself is fine
