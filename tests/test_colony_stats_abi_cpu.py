"""The colony statistics' C-ABI on the host (include/antsrl.h, "The colony statistics"): the entries are declared, exported
and bound, the ABI version stays 5, antsrl_stats_sizes gives the sizes tests/stats_ref.py restates from the header's text,
and every refusal comes before any HIP call: the handles stand over a fake workspace pointer (as in tests/test_abi_cpu.py)
and the blocks are fake addresses, so a call that got as far as a launch would not return ANTSRL_E_INVALID with the
argument's message.  No kernel is launched here.

(The refusal of a row while an Environment.update is in progress needs a handle that has been reset, which takes a
device: tests/test_gpu_colony_stats.py holds it.)"""
import ctypes as C
import os
import re

import pytest

import stats_ref as S
from antsrl_amd import _lib
from antsrl_amd import build as buildmod
from antsrl_amd import config as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("antsrl_stats_sizes", "antsrl_stats_row")
BLOCK = 1 << 20  # a fake, 8-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


def handle(lib, E, W, H, C_, **kw):
    cfg = cm.make_cfg(E, 7, W, H, n_phero=C_, **kw)
    n = C.c_size_t()
    assert lib.antsrl_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
    h = C.c_void_p()
    assert lib.antsrl_create(C.byref(cfg), C.c_void_p(4096), n.value, C.byref(h)) == 0, lib.antsrl_last_error()
    return h


def test_entries_are_declared_exported_and_bound(lib):
    import antsrl_amd
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "antsrl.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, text), "include/antsrl.h does not declare %s" % n
        assert n in _lib.EXPORTS and hasattr(lib, n)
        assert getattr(lib, n).argtypes is not None
    assert re.search(r"#define ANTSRL_ABI_VERSION 5\b", text) and lib.antsrl_abi_version() == 5 and cm.ABI_VERSION == 5
    assert "EpisodeStats" in antsrl_amd.__all__
    from antsrl_amd.stats import EpisodeStats
    assert antsrl_amd.EpisodeStats is EpisodeStats


@pytest.mark.parametrize("C_", [1, 2, 3])
@pytest.mark.parametrize("WH", [(12, 13), (64, 64), (17, 241)], ids=["G156", "G4096", "G4097"])
@pytest.mark.parametrize("E", [1, 9])
def test_sizes_are_the_restated_layout(lib, C_, WH, E):
    W, H = WH
    assert W * H in (156, 4096, 4097)
    h = handle(lib, E, W, H, C_)
    for max_rows in (1, 7):
        rb, sb, tot = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.antsrl_stats_sizes(h, max_rows, C.byref(rb), C.byref(sb), C.byref(tot)) == 0
        assert (rb.value, sb.value, tot.value) == S.layout(E, C_, W * H, max_rows)
        assert lib.antsrl_stats_sizes(h, max_rows, None, None, None) == 0  # (any pointer may be NULL)
        only = C.c_size_t()
        assert lib.antsrl_stats_sizes(h, max_rows, None, C.byref(only), None) == 0 and only.value == sb.value
    lib.antsrl_destroy(h)


def test_every_refusal_comes_before_any_hip_call(lib):
    h = handle(lib, 3, 48, 80, 2)
    blk, st = C.c_void_p(BLOCK), C.c_size_t()

    def refused(rc, *words):
        assert rc == -1, (rc, lib.antsrl_last_error())
        for w in words:
            assert w in lib.antsrl_last_error(), (w, lib.antsrl_last_error())
    # ---- _sizes
    refused(lib.antsrl_stats_sizes(None, 4, None, None, C.byref(st)), b"stats_sizes", b"NULL handle")
    for mr in (0, -1, -(1 << 31)):
        refused(lib.antsrl_stats_sizes(h, mr, None, None, C.byref(st)), b"stats_sizes", b"max_rows")
    # ---- _row
    refused(lib.antsrl_stats_row(None, blk, 4, 0, None), b"stats_row", b"NULL handle")
    refused(lib.antsrl_stats_row(h, None, 4, 0, None), b"stats_row", b"NULL block")
    for mis in (1, 2, 4, 7):
        refused(lib.antsrl_stats_row(h, C.c_void_p(BLOCK + mis), 4, 0, None), b"stats_row", b"8-byte aligned")
    for mr in (0, -1):
        refused(lib.antsrl_stats_row(h, blk, mr, 0, None), b"stats_row", b"max_rows")
    for row, mr in ((-1, 4), (4, 4), (5, 4), (1, 1), (1 << 30, 12)):
        refused(lib.antsrl_stats_row(h, blk, mr, row, None), b"row %d" % row, b"max_rows = %d" % mr)
    # every argument good, the handle never reset: refused by the handle's state, still without a launch
    for row in (0, 3):
        refused(lib.antsrl_stats_row(h, blk, 4, row, None), b"antsrl_reset has not been called")
    refused(lib.antsrl_stats_row(h, C.c_void_p(BLOCK + 8), 4, 0, None), b"antsrl_reset has not been called")  # (8-byte aligned is enough)
    lib.antsrl_destroy(h)
