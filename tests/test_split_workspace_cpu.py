"""The workspace as two blocks (include/antsrl.h: antsrl_workspace_bytes2 / antsrl_create2 / antsrl_workspace_map), host only.

The record block holds the cell records (what the kernels reach with scattered per-cell accesses), the state block
everything else.  For the interleaved layout (c3), separate pheromone buffers behind a radius-3 filter (c4) and the
single-kernel path (k_act, with and without its HBM bit maps):
  * the two sizes add up to the one-block size, and every array of the map is accounted for in exactly one block;
  * the one-block size is what the library reported before the second block existed (the figures below were taken from
    that build), and the one-block map is one gap-free sequence with the records in the middle, where they have always been;
  * no array overlaps another or runs past its block; every offset is 256-byte aligned.
No kernel is launched."""
import ctypes as C

import numpy as np
import pytest

from antsrl_amd import _lib
from antsrl_amd import build as buildmod
from antsrl_amd.config import ACT_SINGLE_KERNEL, CH_ANTS, CH_FOOD, CH_PHERO, CH_WALLS, PHERO_EXPLICIT_SWEEP, make_cfg

RECORD_ARRAYS = {"records", "phero0", "phero1", "food"}


def _gauss7():
    ax = np.arange(-3, 4)
    g = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / 4.5)
    return g / g.sum() * (1 - 0.001)


def _diffuse3():
    f3 = np.ones((3, 3)) * 0.02
    f3[1, 1] = 1 - 8 * 0.02
    return f3 * (1 - 0.001)


_ODD = [(CH_FOOD, 0), (CH_ANTS, 0), (CH_PHERO, 0), (CH_PHERO, 1), (CH_WALLS, 0)]

#: name -> (configuration, antsrl_workspace_bytes of the one-block library, the record arrays expected)
CASES = {
    "c3": (lambda: make_cfg(1024, 512, 256, 256, n_rocks=8, deposit_strength=256.0), 1157742848, {"records"}),
    "c4": (lambda: make_cfg(1024, 512, 256, 256, n_rocks=8, deposit_strength=256.0, filt=_gauss7()), 1694613760,
           {"phero0", "phero1", "food"}),
    "explicit_sweep": (lambda: make_cfg(64, 100, 128, 96, phero_mode=PHERO_EXPLICIT_SWEEP), 20007168, {"phero0", "phero1", "food"}),
    "small_seams": (lambda: make_cfg(3, 40, 16, 12, n_rocks=1, deposit_strength=256.0), 109056, {"records"}),
    "small_radius1": (lambda: make_cfg(2, 40, 16, 16, filt=_diffuse3()), 108288, {"phero0", "phero1", "food"}),
    "k_act": (lambda: make_cfg(4, 64, 64, 48, channels=_ODD), 306688, {"records"}),
    "k_act_pinned": (lambda: make_cfg(3, 40, 16, 12, n_rocks=1, act_path=ACT_SINGLE_KERNEL), 104960, {"records"}),
    "k_act_hbm_maps": (lambda: make_cfg(1, 64, 2048, 2048, channels=_ODD), 69818880, {"records"}),
    "one_channel_scaled": (lambda: make_cfg(2, 16, 32, 32, n_phero=1, channels=[(CH_ANTS, 0), (CH_PHERO, 0), (CH_FOOD, 0)]), 104704,
                           {"phero0", "food"}),
}


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


def _map(lib, cfg, split):
    n = C.c_int32()
    assert lib.antsrl_workspace_map(C.byref(cfg), split, None, 0, C.byref(n)) == 0
    arr = (_lib.AntsWsArray * n.value)()
    m = C.c_int32()
    assert lib.antsrl_workspace_map(C.byref(cfg), split, arr, n.value, C.byref(m)) == 0 and m.value == n.value
    return [(a.name.decode(), a.block, a.offset, a.bytes) for a in arr]


def _r256(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_blocks_account_for_every_array(lib, name):
    mk, parent_bytes, rec_names = CASES[name]
    cfg = mk()
    one, st, rec = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.antsrl_workspace_bytes(C.byref(cfg), C.byref(one)) == 0
    assert one.value == parent_bytes, "antsrl_workspace_bytes changed: %d, was %d" % (one.value, parent_bytes)
    assert lib.antsrl_workspace_bytes2(C.byref(cfg), C.byref(st), C.byref(rec)) == 0
    assert st.value + rec.value == one.value and st.value > 0 and rec.value > 0
    assert lib.antsrl_workspace_bytes2(C.byref(cfg), None, None) == 0  # (either pointer may be NULL)

    single, split = _map(lib, cfg, 0), _map(lib, cfg, 1)
    # one block: ONE sequence without gaps, every array in block 0, the records in the middle (behind walldep_cell)
    off = 0
    for nm, block, o, b in single:
        assert block == 0 and o == off and o % 256 == 0, (nm, block, o, off)
        off += _r256(b)
    assert off == one.value
    names = [nm for nm, _, _, _ in single]
    assert len(set(names)) == len(names)
    first_rec = min(i for i, nm in enumerate(names) if nm in RECORD_ARRAYS)
    assert names[first_rec - 1] == "walldep_cell" and names[first_rec + len(rec_names)] == "walls_bits"

    # two blocks: the same arrays with the same sizes in the same order; records in block 1, everything else in block 0;
    # each block one gap-free sequence from 0 — so nothing overlaps, straddles or runs past its block
    assert [(nm, b) for nm, _, _, b in split] == [(nm, b) for nm, _, _, b in single]
    assert {nm for nm, block, _, _ in split if block == 1} == rec_names
    assert {nm for nm, block, _, _ in split if block == 0} == set(names) - rec_names
    assert not (set(names) - rec_names) & RECORD_ARRAYS
    offs = [0, 0]
    for nm, block, o, b in split:
        assert block in (0, 1) and o == offs[block] and o % 256 == 0, (nm, block, o, offs)
        offs[block] += _r256(b)
    assert offs == [st.value, rec.value]
    for blk in (0, 1):
        spans = sorted((o, o + b) for _, block, o, b in split if block == blk)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= offs[blk]


def test_create2_validates_its_blocks(lib):
    """Host-only argument checks of antsrl_create2 (fake aligned pointers are never dereferenced on the host): missing,
    misaligned, too small and overlapping blocks are refused; the record block may lie below or above the state block."""
    cfg = make_cfg(3, 40, 16, 12, n_rocks=1)
    st, rec = C.c_size_t(), C.c_size_t()
    assert lib.antsrl_workspace_bytes2(C.byref(cfg), C.byref(st), C.byref(rec)) == 0
    h = C.c_void_p()
    S, R = 1 << 20, 1 << 24
    assert lib.antsrl_create2(C.byref(cfg), None, st.value, C.c_void_p(R), rec.value, C.byref(h)) == -1
    assert lib.antsrl_create2(C.byref(cfg), C.c_void_p(S), st.value, None, rec.value, C.byref(h)) == -1
    assert lib.antsrl_create2(C.byref(cfg), C.c_void_p(S + 8), st.value, C.c_void_p(R), rec.value, C.byref(h)) == -1
    assert lib.antsrl_create2(C.byref(cfg), C.c_void_p(S), st.value, C.c_void_p(R + 128), rec.value, C.byref(h)) == -1
    assert b"aligned" in lib.antsrl_last_error()
    assert lib.antsrl_create2(C.byref(cfg), C.c_void_p(S), st.value - 1, C.c_void_p(R), rec.value, C.byref(h)) == -2
    assert b"state block too small" in lib.antsrl_last_error()
    assert lib.antsrl_create2(C.byref(cfg), C.c_void_p(S), st.value, C.c_void_p(R), rec.value - 1, C.byref(h)) == -2
    assert b"record block too small" in lib.antsrl_last_error()
    for r in (S, S + _r256(st.value) - 256, S - _r256(rec.value) + 256):  # the same start, the state's tail, the state's head
        assert lib.antsrl_create2(C.byref(cfg), C.c_void_p(S), st.value, C.c_void_p(r), rec.value, C.byref(h)) == -1
        assert b"overlap" in lib.antsrl_last_error()
    for r in (R, S + st.value, S - _r256(rec.value)):  # far above, right behind, right in front (records below the state)
        assert lib.antsrl_create2(C.byref(cfg), C.c_void_p(S), st.value, C.c_void_p(r), rec.value, C.byref(h)) == 0
        v = C.c_longlong()
        assert lib.antsrl_query(h, 0, C.byref(v)) == 0
        assert lib.antsrl_update(h, None, None) == -1 and b"antsrl_reset" in lib.antsrl_last_error()  # (not reset: nothing is launched)
        lib.antsrl_destroy(h)
    bad = cfg.copy()
    bad.n_phero = 9
    assert lib.antsrl_workspace_bytes2(C.byref(bad), C.byref(st), C.byref(rec)) == -1
    n = C.c_int32()
    assert lib.antsrl_workspace_map(C.byref(cfg), 1, None, 0, None) == -1
    assert lib.antsrl_workspace_map(C.byref(cfg), 1, None, 4, C.byref(n)) == -1
