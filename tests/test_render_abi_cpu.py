"""The episode renderer's C-ABI on the host (include/antsrl.h, "The episode renderer"): the entries are declared and
exported, antsrl_render_sizes gives the sizes the header's text gives, and every refusal comes before any HIP call: the
handles stand over a fake workspace pointer and block, out and scratch are fake addresses (the pattern of
tests/test_recorder_abi_cpu.py), so a call that got as far as a launch would not return ANTSRL_E_INVALID with the
argument's message.  No kernel is launched here."""
import ctypes as C
import os
import re

import pytest

from antsrl_amd import _lib
from antsrl_amd import build as buildmod
from antsrl_amd import config as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("antsrl_render_sizes", "antsrl_render_frames")
SHAPES = [(1, 1, 64, 64, 1, 0), (3, 65, 48, 80, 2, 3), (2, 257, 13, 15, 3, 0)]  # E, N, W, H, C, R
BLOCK, OUT, SCRATCH = 1 << 20, 1 << 24, 1 << 28  # fake, 16-byte aligned device addresses
MAX_ZOOM, MAX_RADIUS = 8, 1024


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


def opts(zoom=3, view=63, ant_radius=1, layer_only=0, phero_max_val=255.0):
    return _lib.AntsRenderOpts(zoom, view, ant_radius, layer_only, phero_max_val)


def test_entries_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "antsrl.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint %s\s*\(" % n, text), "include/antsrl.h does not declare %s" % n
        assert n in _lib.EXPORTS and hasattr(lib, n)
    assert re.search(r"#define ANTSRL_RENDER_MAX_ZOOM %d\b" % MAX_ZOOM, text)
    assert re.search(r"#define ANTSRL_RENDER_MAX_ANT_RADIUS %d\b" % MAX_RADIUS, text)
    assert re.search(r"#define ANTSRL_RENDER_VIEW_ALL 63\b", text)
    m = re.search(r"typedef struct \{(.*?)\} AntsRenderOpts;", text, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == ("int32_t zoom, view_mask, ant_radius, layer_only; double phero_max_val; "
                                                            "uint8_t phero_colors[4][3];")
    assert C.sizeof(_lib.AntsRenderOpts) == 40 and _lib.AntsRenderOpts.phero_max_val.offset == 16 \
        and _lib.AntsRenderOpts.phero_colors.offset == 24


@pytest.mark.parametrize("shape", SHAPES)
def test_sizes_are_what_the_text_gives(lib, shape):
    E, N, W, H, C_, R_ = shape
    h = handle(lib, *shape)
    for S in sorted({1, min(E, 8)}):
        for zoom in (1, 2, 3, 5, MAX_ZOOM):
            fe, sc = C.c_size_t(), C.c_size_t()
            assert lib.antsrl_render_sizes(h, S, C.byref(opts(zoom=zoom)), C.byref(fe), C.byref(sc)) == 0
            assert (fe.value, sc.value) == (3 * W * zoom * H * zoom, 4 * S)
            assert lib.antsrl_render_sizes(h, S, C.byref(opts(zoom=zoom, layer_only=1)), C.byref(fe), C.byref(sc)) == 0
            assert (fe.value, sc.value) == (4 * W * H, 4 * S)
            assert lib.antsrl_render_sizes(h, S, C.byref(opts(zoom=zoom)), None, None) == 0  # (either pointer may be NULL)
    lib.antsrl_destroy(h)


def test_every_refusal_comes_before_any_hip_call(lib):
    h = handle(lib, 3, 65, 48, 80, 2, 3)
    blk, out, scr, fe = C.c_void_p(BLOCK), C.c_void_p(OUT), C.c_void_p(SCRATCH), C.c_size_t()

    def refused(rc, *words):
        assert rc == -1, (rc, lib.antsrl_last_error())
        for w in words:
            assert w in lib.antsrl_last_error(), (w, lib.antsrl_last_error())

    def frames(hh=h, block=blk, n_sel=1, max_frames=4, first=0, count=1, o=None, out_=out, scratch=scr, null_opts=False):
        return lib.antsrl_render_frames(hh, block, n_sel, max_frames, 1, first, count, None if null_opts else C.byref(o or opts()),
                                        out_, scratch, None)

    def sizes(hh=h, n_sel=1, o=None, null_opts=False):
        return lib.antsrl_render_sizes(hh, n_sel, None if null_opts else C.byref(o or opts()), C.byref(fe), None)
    for call in (sizes, frames):  # ---- what both entries check
        refused(call(hh=None), b"NULL handle")
        refused(call(null_opts=True), b"NULL opts")
        for n_sel in (0, -1, 9):
            refused(call(n_sel=n_sel), b"n_sel", b"1..8")
        for zoom in (0, -1, MAX_ZOOM + 1, 1 << 30):
            refused(call(o=opts(zoom=zoom)), b"zoom", b"1..%d" % MAX_ZOOM)
        for ra in (-1, MAX_RADIUS + 1):
            refused(call(o=opts(ant_radius=ra)), b"ant_radius")
        for mv in (0.0, -1.0, float("nan")):
            refused(call(o=opts(phero_max_val=mv)), b"phero_max_val")
        for view in (64, 63 | 128, -1, 1 << 30):
            refused(call(o=opts(view=view)), b"view_mask")
    # ---- _frames: the pointers, the frames and the launch limits
    refused(frames(block=None), b"NULL block")
    refused(frames(out_=None), b"NULL out")
    refused(frames(scratch=None), b"NULL scratch")
    for mis in (1, 4, 8):
        refused(frames(block=C.c_void_p(BLOCK + mis)), b"block must be 16-byte aligned")
        refused(frames(out_=C.c_void_p(OUT + mis)), b"out must be 16-byte aligned")
        refused(frames(scratch=C.c_void_p(SCRATCH + mis)), b"scratch must be 16-byte aligned")
    for mf in (0, -1):
        refused(frames(max_frames=mf), b"max_frames")
    for first, count, mf in ((-1, 1, 4), (0, 0, 4), (0, -2, 4), (0, 5, 4), (3, 2, 4), (4, 1, 4), (1 << 30, 1 << 30, 1 << 30)):
        refused(frames(first=first, count=count, max_frames=mf), b"frames", b"max_frames = %d" % mf)
    refused(frames(count=65536, max_frames=1 << 20), b"launch limits")
    # 48 x 80 cells at zoom 8 (tiles of 32 x 4 cells): 2 * 20 = 40 tiles a frame, 2^24 / (40 * 8) = 52428.8 frames fit; the
    # layer takes 15 workgroups a frame
    refused(frames(n_sel=8, count=52429, max_frames=1 << 20, o=opts(zoom=8)), b"launch limits")
    # every argument good, the handle never reset (no block can have been recorded from it): refused, still without a launch
    refused(frames(n_sel=2, first=1, count=3), b"antsrl_reset has not been called")
    refused(frames(n_sel=8, count=52429, max_frames=1 << 20, o=opts(layer_only=1)), b"antsrl_reset has not been called")
    lib.antsrl_destroy(h)
