"""What the CPU-side checks of the populations' C-ABI entries share (test_population_abi_cpu.py, _explore_, _joint_,
_memory_ and _memory_agent_abi_cpu.py) on top of abi_fakes.py: an AntsPopSpec and the memory net's AntsMemNetShape from
keywords, the call of an entry from a dict of defaults, and the arguments the training entries have in common."""
import ctypes as C

from abi_fakes import FAKE
from antsrl_amd import _lib


def spec(**kw):
    a = dict(P=3, E=6, N=20, base=0, F=294, fmt=1, pitch=0, reserved=0, eps=0.5, lr=1e-3, discount=0.5, seed=7)
    a.update(kw)
    s = _lib.AntsPopSpec(a["P"], a["E"], a["N"], a["base"], a["F"], a["fmt"], a["pitch"], a["reserved"])
    for p in range(max(0, min(a["P"], _lib.POP_MAX))):
        s.members[p] = _lib.AntsPopMember(a["seed"], a["eps"], a["lr"], a["discount"], 0)
    return s


BF16, FP32 = 0, 1  # include/antsrl.h ANTSRL_MEMNET_BF16 / ANTSRL_MEMNET_FP32


def shape(F=294, power=5, mem=20, n_rot=3, n_ph=3, A=2, **kw):
    """The memory net's shape: the widths follow from `power` unless h1, h2 or h3 is given."""
    a = dict(h1=2 ** (1 + power), h2=2 ** (2 + power), h3=2 ** (3 + power))
    a.update(kw)
    return _lib.AntsMemNetShape(F, A, mem, a["h1"], a["h2"], a["h3"], n_rot, n_ph)


def call(entry, s, order, defaults, kw):
    """entry(the spec or NULL, `defaults` updated by `kw` in `order`, a NULL stream)."""
    a = dict(defaults, **kw)
    return entry(C.byref(s) if s is not None else None, *[a[n] for n in order], None)


#: what follows the net's pointers and the ring's arrays in both training entries, and a valid value of each
TRAIN_TAIL = dict(n_rows=200, idx=FAKE, B=48, step=1, beta1=0.9, beta2=0.999, eps=1e-8, grads=FAKE, loss=FAKE, running_loss=FAKE,
                  first=1)


def call_train(entry, s, ptrs, kw, **extra):
    """A training entry: its pointers `ptrs` (all FAKE), TRAIN_TAIL, then `extra` (the explore step's workspace)."""
    defaults = dict({n: FAKE for n in ptrs}, **TRAIN_TAIL, **extra)
    return call(entry, s, ptrs + tuple(TRAIN_TAIL) + tuple(extra), defaults, kw)
