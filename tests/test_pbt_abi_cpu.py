"""CPU-side checks of population-based training's two C-ABI entries (antsrl_pop_fitness / antsrl_pop_exploit;
include/antsrl.h, "Population-based training"): declared, exported and bound, and every invalid argument refused in its own
words before any HIP call.  No kernel is launched here: every call of an entry fails validation or has nothing to copy,
and the pointers are fakes that are never dereferenced (a call that got as far as a launch would not return
ANTSRL_E_INVALID with the message asserted, and without a device not ANTSRL_OK either)."""
import ctypes as C
import os
import re

import pytest

from abi_fakes import INVALID, lib  # noqa: F401 (lib is a fixture)
from antsrl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("antsrl_pop_fitness", "antsrl_pop_exploit")
A = 1 << 20  # a fake, aligned device address


def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "antsrl.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+antsrl_pop_fitness\s*\(\s*const\s+double\s*\*episode_reward,\s*int\s+n_envs,\s*int\s+n_ants,"
                     r"\s*int\s+n_members,\s*double\s*\*row,\s*void\s*\*stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+antsrl_pop_exploit\s*\(\s*int\s+n_arrays,\s*void\s*\*const\s*\*base,\s*const\s+uint64_t\s*\*row_bytes,"
                     r"\s*int\s+n_members,\s*int\s+n_pairs,\s*const\s+int32_t\s*\*src,\s*const\s+int32_t\s*\*dst,\s*void\s*\*stream\s*\)\s*;", text)
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.EXPORTS, n
    vp, i32 = C.c_void_p, C.c_int
    assert lib.antsrl_pop_fitness.argtypes == [vp, i32, i32, i32, vp, vp]
    assert lib.antsrl_pop_exploit.argtypes == [i32, C.POINTER(vp), C.POINTER(C.c_uint64), i32, i32, C.POINTER(C.c_int32),
                                               C.POINTER(C.c_int32), vp]
    assert lib.antsrl_abi_version() == 5  # the entries are additive


def refused(lib, rc, message):
    assert rc == INVALID, (rc, lib.antsrl_last_error())
    assert lib.antsrl_last_error() == message, (lib.antsrl_last_error(), message)


# ---- antsrl_pop_fitness
def fitness(lib, er=A, E=8, N=5, P=4, row=A + (1 << 16)):
    return lib.antsrl_pop_fitness(er, E, N, P, row, None)


@pytest.mark.parametrize("kw,message", [
    (dict(er=None), b"pop_fitness: episode_reward is required"),
    (dict(row=None), b"pop_fitness: row is required"),
    (dict(er=A + 4), b"pop_fitness: episode_reward must be 8-byte aligned"),
    (dict(row=A + 4), b"pop_fitness: row must be 8-byte aligned"),
    (dict(P=0), b"pop_fitness: n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    (dict(P=65, E=65), b"pop_fitness: n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    (dict(E=0), b"pop_fitness: n_envs and n_ants must be >= 1 (0, 5)"),
    (dict(N=0), b"pop_fitness: n_envs and n_ants must be >= 1 (8, 0)"),
    (dict(N=-3), b"pop_fitness: n_envs and n_ants must be >= 1 (8, -3)"),
    (dict(E=9), b"pop_fitness: n_envs = 9 is not a multiple of n_members = 4 (members own equal shares)"),
    (dict(row=A), b"pop_fitness: row overlaps episode_reward"),
    (dict(row=A + 8 * 5 * 8 - 8), b"pop_fitness: row overlaps episode_reward"),        # its first word is the block's last
    (dict(er=A + 4 * 24 - 8, row=A), b"pop_fitness: row overlaps episode_reward"),     # its last word is the block's first
], ids=["null_reward", "null_row", "odd_reward", "odd_row", "p0", "p65", "e0", "n0", "n_negative", "not_a_multiple", "same",
        "row_at_the_end", "row_in_front"])
def test_fitness_refusals(lib, kw, message):
    refused(lib, fitness(lib, **kw), message)


def test_fitness_checks_in_the_documented_order(lib):
    """NULL pointers, then n_members, then the batch, then the shares, then the overlap."""
    refused(lib, lib.antsrl_pop_fitness(None, 0, 0, 0, None, None), b"pop_fitness: episode_reward is required")
    refused(lib, lib.antsrl_pop_fitness(A, 0, 0, 0, A, None), b"pop_fitness: n_members must be in [1, ANTSRL_POP_MAX = 64] (0)")
    refused(lib, lib.antsrl_pop_fitness(A, 0, 5, 4, A, None), b"pop_fitness: n_envs and n_ants must be >= 1 (0, 5)")
    refused(lib, lib.antsrl_pop_fitness(A, 9, 5, 4, A, None), b"pop_fitness: n_envs = 9 is not a multiple of n_members = 4 (members own equal shares)")


# ---- antsrl_pop_exploit
def exploit(lib, bases=(A, A + (1 << 16)), rows=(38412, 7128), P=6, src=(0, 0, 1), dst=(2, 3, 5), n_arrays=None, n_pairs=None,
            null=()):
    n = len(bases)
    base = (C.c_void_p * max(1, n))(*bases)
    row_bytes = (C.c_uint64 * max(1, n))(*rows)
    s, d = (C.c_int32 * max(1, len(src)))(*src), (C.c_int32 * max(1, len(dst)))(*dst)
    args = dict(base=base, row_bytes=row_bytes, src=s, dst=d)
    for name in null:
        args[name] = None
    return lib.antsrl_pop_exploit(n if n_arrays is None else n_arrays, args["base"], args["row_bytes"], P,
                                  len(src) if n_pairs is None else n_pairs, args["src"], args["dst"], None)


@pytest.mark.parametrize("kw,message", [
    (dict(n_arrays=0), b"pop_exploit: n_arrays must be in [1, ENV_COPY_MAX_ARRAYS = 40] (0)"),
    (dict(n_arrays=41), b"pop_exploit: n_arrays must be in [1, ENV_COPY_MAX_ARRAYS = 40] (41)"),
    (dict(n_pairs=-1), b"pop_exploit: n_pairs must be in [0, ENV_COPY_MAX_PAIRS = 640] (-1)"),
    (dict(n_pairs=641), b"pop_exploit: n_pairs must be in [0, ENV_COPY_MAX_PAIRS = 640] (641)"),
    (dict(P=0), b"pop_exploit: n_members must be in [1, ANTSRL_POP_MAX = 64] (0)"),
    (dict(P=65), b"pop_exploit: n_members must be in [1, ANTSRL_POP_MAX = 64] (65)"),
    (dict(null=("base",)), b"pop_exploit: NULL base or row_bytes"),
    (dict(null=("row_bytes",)), b"pop_exploit: NULL base or row_bytes"),
    (dict(rows=(38412, 0)), b"pop_exploit: row_bytes[1] is 0"),
    (dict(bases=(None, A)), b"pop_exploit: base[0] is NULL"),
    (dict(null=("src",)), b"pop_exploit: NULL src or dst"),
    (dict(null=("dst",)), b"pop_exploit: NULL src or dst"),
    (dict(src=(0, -1, 1)), b"pop_exploit: src[1] = -1 is not in [0, 6)"),
    (dict(src=(0, 0, 6)), b"pop_exploit: src[2] = 6 is not in [0, 6)"),
    (dict(dst=(-2, 3, 5)), b"pop_exploit: dst[0] = -2 is not in [0, 6)"),
    (dict(dst=(2, 3, 6)), b"pop_exploit: dst[2] = 6 is not in [0, 6)"),
    (dict(dst=(2, 3, 2)), b"pop_exploit: dst 2 appears twice (dst[2])"),
    (dict(src=(0, 3, 1)), b"pop_exploit: member 3 is a src (src[1]) and a dst"),
    (dict(src=(4,), dst=(4,)), b"pop_exploit: member 4 is a src (src[0]) and a dst"),
], ids=["no_array", "too_many_arrays", "pairs_negative", "too_many_pairs", "p0", "p65", "null_base", "null_row_bytes", "row_bytes_0",
        "null_base_entry", "null_src", "null_dst", "src_negative", "src_out_of_range", "dst_negative", "dst_out_of_range",
        "dst_twice", "dst_in_src", "onto_itself"])
def test_exploit_refusals(lib, kw, message):
    refused(lib, exploit(lib, **kw), message)


def test_no_pair_is_ok_and_launches_nothing(lib):
    """n_pairs == 0 returns ANTSRL_OK (src and dst may be NULL then), after the arrays have been checked."""
    assert exploit(lib, src=(), dst=()) == 0
    assert exploit(lib, src=(), dst=(), null=("src", "dst")) == 0
    refused(lib, exploit(lib, src=(), dst=(), rows=(0, 8)), b"pop_exploit: row_bytes[0] is 0")
    # the widest table passes the arrays' checks (a list of pairs that passes too would launch: tests/test_gpu_pbt_exploit.py)
    assert exploit(lib, bases=tuple(A + (i << 16) for i in range(40)), rows=tuple(4 + i for i in range(40)), src=(), dst=()) == 0
