"""The episode recorder's C-ABI on the host (include/antsrl.h, "The episode recorder"): the entries are declared and
exported, antsrl_recorder_sizes gives the layout tests/recorder_ref.py restates from the header's text, every section of
every frame is 16-byte aligned, and every refusal comes before any HIP call: the handles stand over a fake workspace
pointer (as in tests/test_abi_cpu.py) and the blocks are fake addresses, so a call that got as far as a launch would
not return ANTSRL_E_INVALID with the argument's message.  No kernel is launched here.

(The refusal of a call while an Environment.update is in progress needs a handle that has been reset, which takes a
device: tests/test_gpu_recorder.py holds it.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import recorder_ref as R
from antsrl_amd import _lib
from antsrl_amd import build as buildmod
from antsrl_amd import config as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("antsrl_recorder_sizes", "antsrl_recorder_begin", "antsrl_recorder_frame")
SHAPES = [(1, 1, 64, 64, 1, 0), (3, 65, 48, 80, 2, 3), (2, 257, 64, 64, 3, 0)]  # E, N, W, H, C, R
BLOCK = 1 << 20  # a fake, 16-byte aligned device address


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


def handle(lib, E, N, W, H, C_, R_, **kw):
    cfg = cm.make_cfg(E, N, W, H, n_phero=C_, n_rocks=R_, **kw)
    n = C.c_size_t()
    assert lib.antsrl_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
    h = C.c_void_p()
    assert lib.antsrl_create(C.byref(cfg), C.c_void_p(4096), n.value, C.byref(h)) == 0, lib.antsrl_last_error()
    return h


def idx(*v):
    return (C.c_int32 * len(v))(*v)


def test_entries_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "antsrl.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, text), "include/antsrl.h does not declare %s" % n
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert re.search(r"#define ANTSRL_RECORDER_MAX_ENVS 8\b", text)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("heatmap", [1, 0])
@pytest.mark.parametrize("reward", [cm.REWARD_EXPLORATION, cm.REWARD_ALL, cm.REWARD_FOOD, cm.REWARD_NONE])
def test_sizes_are_the_restated_layout(lib, shape, heatmap, reward):
    E, N, W, H, C_, R_ = shape
    h = handle(lib, *shape, reward_kind=reward)
    explored = bool(heatmap) and reward in (cm.REWARD_EXPLORATION, cm.REWARD_ALL)
    for S in sorted({1, min(E, 8)}):
        for max_frames in (1, 7):
            st, fr, tot = C.c_size_t(), C.c_size_t(), C.c_size_t()
            assert lib.antsrl_recorder_sizes(h, S, max_frames, heatmap, C.byref(st), C.byref(fr), C.byref(tot)) == 0
            assert (st.value, fr.value, tot.value) == R.sizes(S, N, W, H, C_, R_, explored, max_frames)
            # the sections restated one by one add up to the header's formulas
            assert S * sum(s[3] for s in R.static_sections(N, W, H, C_, R_)) == st.value
            assert S * sum(s[3] for s in R.frame_sections(N, W, H, C_, R_, explored)) == fr.value
            assert lib.antsrl_recorder_sizes(h, S, max_frames, heatmap, None, None, None) == 0  # (any pointer may be NULL)
    lib.antsrl_destroy(h)


@pytest.mark.parametrize("shape", SHAPES + [(2, 7, 12, 13, 2, 1), (2, 5, 13, 15, 2, 0)])
@pytest.mark.parametrize("explored", [True, False])
def test_every_section_of_every_frame_is_16_byte_aligned(shape, explored):
    E, N, W, H, C_, R_ = shape
    offs = R.section_offsets(min(E, 8), N, W, H, C_, R_, explored, 3)
    assert len(offs) == min(E, 8) * (3 + 3 * (8 + C_ + (1 if explored else 0)))
    for what, where, name, off in offs:
        assert off % 16 == 0, (what, where, name, off)


def test_every_refusal_comes_before_any_hip_call(lib):
    E = 3
    h = handle(lib, E, 65, 48, 80, 2, 3)
    blk, one, st = C.c_void_p(BLOCK), idx(0), C.c_size_t()

    def refused(rc, *words):
        assert rc == -1, (rc, lib.antsrl_last_error())
        for w in words:
            assert w in lib.antsrl_last_error(), (w, lib.antsrl_last_error())
    # ---- _sizes
    refused(lib.antsrl_recorder_sizes(None, 1, 4, 1, None, None, C.byref(st)), b"NULL handle")
    for n_sel in (0, -1, 9):
        refused(lib.antsrl_recorder_sizes(h, n_sel, 4, 1, None, None, C.byref(st)), b"n_sel", b"1..8")
    for mf in (0, -3):
        refused(lib.antsrl_recorder_sizes(h, 1, mf, 1, None, None, C.byref(st)), b"max_frames")
    # ---- _begin and _frame: the same checks, in front of the handle's state
    for name, call in (("begin", lambda *a: lib.antsrl_recorder_begin(*a, None)),
                       ("frame", lambda *a: lib.antsrl_recorder_frame(*a, 0, None))):
        refused(call(None, blk, one, 1, 4, 1), b"NULL handle")
        refused(call(h, None, one, 1, 4, 1), b"NULL block")
        for mis in (1, 4, 8):
            refused(call(h, C.c_void_p(BLOCK + mis), one, 1, 4, 1), b"16-byte aligned")
        for n_sel in (0, -1, 9):
            refused(call(h, blk, idx(0, 1, 2, 0, 1, 2, 0, 1, 2), n_sel, 4, 1), b"n_sel", b"1..8")
        refused(call(h, blk, None, 1, 4, 1), b"env_indices")
        for bad in ((E,), (-1,), (0, E), (2, 1, 1 << 30)):
            refused(call(h, blk, idx(*bad), len(bad), 4, 1), b"env_indices", b"n_envs = 3")
        for rep in ((0, 0), (2, 1, 2), (1, 0, 2, 1)):
            refused(call(h, blk, idx(*rep), len(rep), 4, 1), b"repeats environment")
        for mf in (0, -1):
            refused(call(h, blk, one, 1, mf, 1), b"max_frames")
        # every argument good, the handle never reset: refused by the handle's state, still without a launch
        refused(call(h, blk, idx(2, 0), 2, 4, 1), b"antsrl_reset has not been called")
    # ---- _frame: the frame's slot
    for frame, mf in ((-1, 4), (4, 4), (5, 4), (1, 1), (1 << 30, 12)):
        refused(lib.antsrl_recorder_frame(h, blk, one, 1, mf, 1, frame, None), b"frame", b"max_frames = %d" % mf)
    refused(lib.antsrl_recorder_frame(h, blk, one, 1, 4, 1, 3, None), b"antsrl_reset has not been called")  # (3 of 4 fits)
    lib.antsrl_destroy(h)


def test_the_restated_cast():
    v = np.array([0, 0.99, 1, 254.999, 255, 255.5, 256, 1e9], dtype=np.float32)
    assert R.cast_u8(v).tolist() == [0, 0, 1, 254, 255, 255, 255, 255]
    assert R.cast_u8(v).dtype == np.uint8
    below = v[v < 256]
    assert np.array_equal(R.cast_u8(below), below.astype(np.uint8))  # numpy's astype there; from 256 up it is the header's rule
    every = np.arange(0, 256 * 8, dtype=np.float32) / 8  # every eighth below 256
    assert np.array_equal(R.cast_u8(every), every.astype(np.uint8))
