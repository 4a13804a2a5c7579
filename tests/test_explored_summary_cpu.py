"""The explored summary's index arithmetic (antsrl_amd/csrc/antsrl_explored.h: one bit per tile of 8 x 8 cells, and the per-ant
test "every tile the patch can touch has its bit") checked on the host with the SAME functions the kernels use: g++ compiles
the header (tests/native/explored_check.cpp).

SOUNDNESS OF THE BOX.  For every pose, each of the 49 cells RL_api.py:110-119 perceives (rotate the 7 x 7 offsets by
theta + pi/2, add the centre shifted by fwd_delta along the heading, round half to even, wrap) lies in a tile the per-ant test
inspects — so an ant that passes the test cannot perceive a cell of a tile without its bit.  Poses: random ones, headings in
multiples of 40 degrees, centres on .5 boundaries and at the grid's wrap; grids 8 x 8, 16 x 16, 32 x 64, 256 x 256; delta 1.1,
fwd_delta 4 (the reference's values).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
R, DELTA, FWD = 3, 1.1, 4.0
GRIDS = [(8, 8), (16, 16), (32, 64), (256, 256)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("explored") / "explored_check.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", os.path.join(HERE, "native", "explored_check.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.expl_box_margin.restype = C.c_double
    lib.expl_box_margin.argtypes = [C.c_int, C.c_double]
    lib.expl_box.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.expl_box_full.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]
    lib.expl_check_poses.restype = C.c_long
    lib.expl_check_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_long)]
    for f in (lib.expl_tile_count, lib.expl_tile_index, lib.expl_tile_word, lib.expl_tile_bit):
        f.restype = C.c_uint
    return lib


def poses(W, H, rng):
    """[n][3] ant poses x, y, theta: random, and the adversarial families of the module's text."""
    n = 4000
    rnd = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(0, 2 * np.pi, n)], axis=1)
    th40 = np.deg2rad(40.0) * np.arange(9)
    edge = np.array([0.0, 0.5, 1.0, 1.5, 3.5, 4.5, 7.5, 8.0, 8.5, W - 0.5, W - 1e-9, W / 2 - 0.5, W / 2, np.nextafter(W, 0)])
    edge, edge_y = edge % W, edge % H
    adv = np.array([(x, y, t) for x, y in zip(edge, edge_y) for t in np.concatenate([th40, [np.pi / 4, np.pi / 2, 3 * np.pi / 4]])])
    # centres (not ants) on .5 boundaries: place the ant so that the shifted centre lands there
    half = np.array([(cx - np.cos(t) * FWD, cy - np.sin(t) * FWD, t) for cx in (0.5, 8.5, W - 0.5) for cy in (0.5, 7.5, H - 0.5) for t in th40])
    half[:, 0] %= W
    half[:, 1] %= H
    return np.concatenate([rnd, adv, half])


def perceive_cells(p, W, H):
    """RL_api.py:100-119 for poses p: the frame centres [n][2] and the wrapped integer cells [n][49][2]."""
    x, y, th = p[:, 0], p[:, 1], p[:, 2]
    cxy = np.stack([x + np.cos(th) * FWD, y + np.sin(th) * FWD], axis=1)
    t_f = th + np.pi * 0.5
    ct, st = np.cos(t_f), np.sin(t_f)
    ar = np.arange(-R, R + 1).astype(float) * DELTA
    ox, oy = np.meshgrid(ar, ar)  # coords[a][b] = (arange[b], arange[a])
    ox, oy = ox.ravel()[None, :], oy.ravel()[None, :]
    rx = ct[:, None] * ox - st[:, None] * oy
    ry = st[:, None] * ox + ct[:, None] * oy
    ix = np.mod(np.round(rx + cxy[:, :1]).astype(np.int64), W)
    iy = np.mod(np.round(ry + cxy[:, 1:]).astype(np.int64), H)
    return np.ascontiguousarray(cxy), np.ascontiguousarray(np.stack([ix, iy], axis=2).astype(np.int32))


@pytest.mark.parametrize("W,H", GRIDS)
def test_tile_bits_are_a_bijection_onto_the_first_bits(lib, W, H):
    assert lib.expl_tiles_ok(W, H) == 1
    nt = lib.expl_tile_count(W, H)
    assert nt == (W // 8) * (H // 8)
    seen = {}
    for x in range(W):
        for y in range(H):
            t = lib.expl_tile_index(x, y, H)
            assert t < nt
            seen.setdefault(t, set()).add((x // 8, y // 8))
    assert sorted(seen) == list(range(nt)) and all(len(v) == 1 for v in seen.values())
    places = {(lib.expl_tile_word(t), lib.expl_tile_bit(t)) for t in range(nt)}
    assert len(places) == nt and all(w * 32 + b == t for t, (w, b) in zip(range(nt), sorted(places)))
    assert max(w for w, _ in places) < (W * H + 31) // 32  # inside the environment's explored_bits slice


def test_grids_without_tiles_are_refused(lib):
    for W, H in ((4, 8), (8, 4), (4, 4), (24, 32), (32, 24), (1, 1)):
        assert lib.expl_tiles_ok(W, H) == 0


@pytest.mark.parametrize("W,H", GRIDS)
def test_every_perceived_cell_lies_in_an_inspected_tile(lib, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    p = poses(W, H, rng)
    cxy, cells = perceive_cells(p, W, H)
    margin = lib.expl_box_margin(R, DELTA)
    assert margin == R * DELTA * 1.4142135623730951 + 0.5
    nt = lib.expl_tile_count(W, H)
    nwords = (W * H + 31) // 32
    for fill in (0.0, 0.9, 1.0):  # no bit, most bits, every bit
        tiles = rng.uniform(size=nt) < fill if fill < 1.0 else np.ones(nt, bool)
        bits = np.zeros(nwords, np.uint32)
        for t in np.nonzero(tiles)[0]:
            bits[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
        full = np.zeros(len(p), np.uint8)
        n_small = C.c_long()
        bad = lib.expl_check_poses(bits.ctypes.data, cxy.ctypes.data, cells.ctypes.data, len(p), 49, margin, W, H, full.ctypes.data, C.byref(n_small))
        assert bad < 1 << 40, "the small-box form disagrees with the general one on %d poses" % (bad >> 40)
        assert bad == 0, "%d perceived cells outside their ant's box" % bad
        assert n_small.value == len(p), "the reference's patch is a small box on every grid"
        # the verdict itself, restated: full <=> every tile of the box has its bit; and then every perceived cell's tile has
        out = (C.c_int * 4)()
        for i in range(0, len(p), 7):
            lib.expl_box(cxy[i, 0], cxy[i, 1], margin, W, H, out)
            tx0, ntx, ty0, nty = list(out)
            assert 1 <= ntx <= W // 8 and 1 <= nty <= H // 8
            want = all(tiles[((tx0 + a) % (W // 8)) * (H // 8) + (ty0 + b) % (H // 8)] for a in range(ntx) for b in range(nty))
            assert bool(full[i]) == want, (i, p[i], list(out))
        cell_tiles = (cells[:, :, 0] // 8) * (H // 8) + cells[:, :, 1] // 8
        assert tiles[cell_tiles[full.astype(bool)]].all()
        if fill == 0.0:
            assert not full.any()
        if fill == 1.0:
            assert full.all()


def test_the_box_at_the_reference_size_reads_three_tiles_per_axis_at_most(lib):
    W = H = 256
    margin = lib.expl_box_margin(R, DELTA)
    out = (C.c_int * 4)()
    rng = np.random.default_rng(5)
    for cx, cy in rng.uniform(-4, 260, (2000, 2)):
        lib.expl_box(cx, cy, margin, W, H, out)
        assert 2 <= out[1] <= 3 and 2 <= out[3] <= 3
