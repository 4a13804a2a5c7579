"""antsrl_render_frames (antsrl_amd/render.py; include/antsrl.h, "The episode renderer") against tests/render_ref.py, byte
for byte: the colour layer (layer_only) and the full frames, with sentinel bytes around `out` and `scratch` intact and
the recorder's block unchanged.

Two kinds of case (CASES; a chosen list, not the full product):
  packed     the block is built by render_ref.pack_block from arrays chosen here: dense random planes, planes of all 255
             and of all 0; ants on all four borders and in all four corners, three ants on ONE pixel with three
             reward_states (the highest index must win), holding on and off, a rock straddling the left edge and one
             over the bottom right corner
  recorded   three real steps of a small environment, recorded as tests/test_gpu_recorder.py records them — one of them
             with REWARD_FOOD, where the block has no explored section
Shapes: grids 12 x 13 and 13 x 15 (narrower than a tile's 32 cells, no multiple of 4 either way: a tile is 32 cells by 32,
16, 8 or 4 with the zoom), 48 x 80 and 64 x 64 (several tiles, 48 no multiple of 32); zoom 1, 2, 3, 5 and 8 (the maximum,
and one zoom of each tile height); S = 1, 2, 8; N = 1, 65, 257; C = 1, 2, 3; R = 0, 3; first > 0 with count < n_frames;
each view bit cleared alone; ant_radius 0 and 300 (a tile is at most 256 pixels across).  `-s` prints one MEASURED line per kernel."""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import render_ref as RR

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5
COLOURS = ((255, 64, 0), (64, 64, 255), (100, 255, 100), (255, 255, 64))


def case(W, H, S=1, N=65, Cn=2, R=0, zoom=3, view=63, ra=1, frames=2, first=0, count=None, planes="random", explored=True):
    return SimpleNamespace(W=W, H=H, S=S, N=N, C=Cn, R=R, zoom=zoom, view=view, ra=ra, frames=frames, first=first,
                           count=frames - first if count is None else count, planes=planes, explored=explored)


CASES = {
    "12x13-z1-one-ant-r0": case(12, 13, N=1, Cn=1, zoom=1, ra=0),
    "13x15-z2-s2-rocks": case(13, 15, S=2, Cn=2, R=3, zoom=2),
    "13x15-z3-all-255": case(13, 15, Cn=3, R=3, zoom=3, planes="255"),
    "13x15-z3-all-0": case(13, 15, Cn=2, zoom=3, planes="0"),
    "13x15-z8-radius-300": case(13, 15, Cn=2, R=3, zoom=8, ra=300, frames=1),
    "48x80-z3-s8-first-1": case(48, 80, S=8, Cn=3, R=3, zoom=3, ra=2, frames=4, first=1, count=2),
    "48x80-z1-no-explored": case(48, 80, S=2, N=257, Cn=1, zoom=1, ra=1, explored=False),
    "64x64-z5-n257": case(64, 64, N=257, Cn=2, zoom=5, ra=2),
    "64x64-z8-s2-rocks": case(64, 64, S=2, N=257, Cn=2, R=3, zoom=8, ra=4, frames=1),
    "64x64-z2-r0": case(64, 64, N=65, Cn=2, R=3, zoom=2, ra=0, frames=1),
}
for _bit in range(6):
    CASES["13x15-z3-without-view-%d" % _bit] = case(13, 15, Cn=2, R=3, zoom=3, ra=2, view=63 & ~(1 << _bit), frames=1)
RECORDED = {  # name: (E, N, W, H, make_cfg keywords, selection, zoom, ant_radius)
    "recorded-default": (3, 50, 64, 64, {}, [2, 0], 3, 1),
    "recorded-reward-food": (3, 50, 64, 64, dict(reward_kind=2), [0], 2, 1),
    "recorded-rocks-48x80": (4, 65, 48, 80, dict(n_rocks=3), [3], 1, 0),
}


def make_env(E, N, W, H, kw, seed=5):
    """A small environment, as tests/test_gpu_recorder.py makes it."""
    from antsrl_amd import config as cm
    from antsrl_amd.batched import BatchedAntsEnv
    from antsrl_amd.synth import synth_init
    cfg = cm.make_cfg(E, N, W, H, deposit_strength=256.0, max_time=2000, **kw)
    env = BatchedAntsEnv(cfg)
    small = min(W, H) < 32
    env.reset(synth_init(cfg, seed=seed, n_food_discs=6, food_rmin=1 if small else 3, food_rmax=3 if small else 6))
    return env


def chosen_arrays(c, rng):
    """The static part and the frames of a packed case."""
    n, S, N, W, H = c.frames, c.S, c.N, c.W, c.H
    if c.planes == "random":
        plane = lambda *shape: rng.integers(0, 256, shape).astype(np.uint8)  # noqa: E731
    else:
        plane = lambda *shape: np.full(shape, int(c.planes), dtype=np.uint8)  # noqa: E731
    xyt = np.stack([rng.uniform(0, W, (n, S, N)), rng.uniform(0, H, (n, S, N)), rng.uniform(-3, 3, (n, S, N))], axis=-1)
    edge = [(0.0, 0.0), (W - 0.01, 0.0), (0.0, H - 0.01), (W - 0.01, H - 0.01),          # the corners
            (W / 2, 0.0), (W / 2, H - 0.01), (0.0, H / 2), (W - 0.01, H / 2),              # the borders
            (W / 3 + 0.300, H / 3 + 0.300), (W / 3 + 0.301, H / 3 + 0.302), (W / 3 + 0.302, H / 3 + 0.301)]  # one pixel, three ants
    for i, (x, y) in enumerate(edge[:N]):
        xyt[:, :, N - 1 - i, 0], xyt[:, :, N - 1 - i, 1] = x, y  # (the highest indices: nothing random draws over them)
    reward_state = rng.integers(0, 256, (n, S, N)).astype(np.uint8)
    holding = (rng.random((n, S, N)) < 0.5).astype(np.float32) * 2.5
    if N > len(edge):
        reward_state[:, :, N - 11:N - 8] = (240, 60, 150)
        holding[:, :, N - 11:N - 8] = (0.0, 1.0, 0.0)
    rock_centers = np.zeros((n, S, c.R, 2))
    rock_rw = np.zeros((S, c.R, 2))
    if c.R:
        rock_centers[:] = np.array([(0.5, H / 2), (W - 1.0, H - 0.2), (W / 2 + 0.25, H / 4 + 0.5)])[:c.R]
        rock_centers += rng.uniform(-0.2, 0.2, rock_centers.shape)
        rock_rw[:] = np.array([(2.5, 1.0), (1.7, 2.0), (1.2, 1.0)])[:c.R]
    static = dict(anthill_xyr=np.tile(np.array([W // 3, H // 2, 3], dtype=np.int32), (S, 1)), rock_rw=rock_rw,
                  walls=(rng.random((S, W, H)) < 0.1).astype(np.uint8))
    frames = dict(timestep=np.arange(2, 2 + n, dtype=np.int32)[:, None].repeat(S, axis=1), anthill_food=np.zeros((n, S)),
                  rock_centers=rock_centers, ants_xyt=xyt, holding=holding, mandibles=(holding > 0).astype(np.uint8),
                  reward_state=reward_state, phero=plane(n, S, c.C, W, H), food=plane(n, S, W, H))
    if c.explored:
        frames["explored"] = (rng.random((n, S, W, H)) < 0.5).astype(np.uint8)
    return static, frames


def guarded(nbytes, device):
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD: GUARD + nbytes]


def launch(ren, layer_only, first, count):
    """antsrl_render_frames into guarded `out` and `scratch`: the picture on the host, the kernels' time, the guards checked."""
    import torch
    from antsrl_amd import _lib
    from antsrl_amd._lib import ptr
    rec, c, Z = ren.rec, ren.cfg, ren.zoom
    o = ren._opts(layer_only)
    shape = (count, ren.S, c.w, c.h, 4) if layer_only else (count, ren.S, c.h * Z, c.w * Z, 3)
    assert ren._frame_env_bytes == int(np.prod(shape[2:]))
    obuf, out = guarded(int(np.prod(shape)), rec.device)
    sbuf, scratch = guarded(count * ren._scratch_per_frame, rec.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    _lib.check(ren._lib.antsrl_render_frames(rec.env._h, ptr(rec.block), ren.S, rec.max_frames, int(rec.with_heatmap), first, count,
                                             C.byref(o), ptr(out), ptr(scratch), rec.env._stream()), "render_frames")
    t1.record()
    torch.cuda.synchronize()
    for buf, used in ((obuf, out.numel()), (sbuf, scratch.numel())):
        host = buf.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[GUARD + used:] == FILL).all(), "a guard byte was written"
    fmax = scratch.cpu().numpy().view(np.int32).reshape(count, ren.S)
    return out.cpu().numpy().reshape(shape), fmax, t0.elapsed_time(t1)


def compare(name, ren, f, first, count, view, ra):
    """Both modes against render_ref, through the entry (guards) and through the class."""
    rec = ren.rec
    before = rec.block.clone()
    colours, mv, Z = COLOURS[:ren.cfg.n_phero], ren.phero_max_val, ren.zoom
    lay, fmax, ms_l = launch(ren, True, first, count)
    img, _, ms_f = launch(ren, False, first, count)
    print("MEASURED %s: k_render_food_max + k_render_layer %.3f ms, k_render_food_max + k_render_frames %.3f ms for %d frame(s) "
          "x %d env(s), %d x %d cells, zoom %d (one call each, by device events)" % (name, ms_l, ms_f, count, ren.S, ren.cfg.w, ren.cfg.h, Z))
    assert np.array_equal(fmax, f["food"][first: first + count].reshape(count, ren.S, -1).max(axis=2))
    want_lay = RR.layer_frames(f, first, count, colours, mv, view)
    assert lay.shape == want_lay.shape and np.array_equal(lay, want_lay), "colour layer: %d bytes differ" % (lay != want_lay).sum()
    want = RR.render_frames(f, first, count, colours, mv, Z, view, ra)
    assert img.shape == want.shape
    assert np.array_equal(img, want), "frames: %d bytes differ, first at %s" % ((img != want).sum(), np.argwhere(img != want)[:3].tolist())
    import torch
    assert torch.equal(rec.block, before), "the block changed"
    assert np.array_equal(ren.colour_layer(first, count).cpu().numpy(), want_lay)
    assert np.array_equal(ren.render(first, count).cpu().numpy(), want)
    return img


@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_blocks_render_to_the_bytes_of_render_ref(name):
    import torch
    from antsrl_amd.recorder import EpisodeRecorder
    from antsrl_amd.render import EpisodeRenderer
    c = CASES[name]
    kw = dict(n_phero=c.C, n_rocks=c.R)
    if not c.explored:
        kw["reward_kind"] = 2  # REWARD_FOOD: no explored section
    env = make_env(c.S, c.N, c.W, c.H, kw)
    rec = EpisodeRecorder(env, env_indices=list(range(c.S)), max_frames=c.frames, phero_colors=COLOURS)
    assert rec.has_heatmap == c.explored
    static, frames = chosen_arrays(c, np.random.default_rng(zlib.crc32(name.encode())))
    packed = RR.pack_block(rec.static_fields, rec.frame_fields, c.S, static, frames)
    assert packed.size == rec.bytes
    rec.block.copy_(torch.from_numpy(packed).to(rec.device))
    rec.n_frames, rec._begun = c.frames, True
    f = rec.frames()
    for k, v in {**static, **frames}.items():  # the packer and the product's decoding agree on the layout
        assert np.array_equal(f[k], np.asarray(v, dtype=f[k].dtype)), k
    ren = EpisodeRenderer(rec, zoom=c.zoom, view=c.view, ant_radius=c.ra, phero_max_val=255.0)
    img = compare(name, ren, f, c.first, c.count, c.view, c.ra)
    if c.N > 11 and c.view & 2 and c.ra <= 4:  # the three ants on one pixel: the highest index wins
        Z = c.zoom
        px, py = int((c.W / 3 + 0.30) * Z), int((c.H / 3 + 0.30) * Z)
        for i in (c.N - 9, c.N - 10, c.N - 11):
            assert (int(frames["ants_xyt"][0, 0, i, 0] * Z), int(frames["ants_xyt"][0, 0, i, 1] * Z)) == (px, py)
        rs = int(frames["reward_state"][c.first, 0, c.N - 9])  # 150, not holding
        assert img[0, 0, py, px].tolist() == [rs, rs, int(128 * rs / 255.0)]


@functools.lru_cache(maxsize=None)
def recorded(name):
    import torch
    from antsrl_amd.recorder import EpisodeRecorder
    E, N, W, H, kw, sel, zoom, ra = RECORDED[name]
    env = make_env(E, N, W, H, kw)
    rec = EpisodeRecorder(env, env_indices=sel, max_frames=3, phero_colors=COLOURS)
    g = torch.Generator(device=env.device).manual_seed(11)
    rot = torch.randint(-1, 2, (3, E, N), generator=g, device=env.device, dtype=torch.int8)
    ph = torch.randint(0, 3, (3, E, N), generator=g, device=env.device, dtype=torch.int8)
    rec.begin()
    for t in range(3):
        env.step_update(rot[t], ph[t])
        rec.record()
    return rec, rec.frames()


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_recorded_steps_render_to_the_bytes_of_render_ref(name):
    from antsrl_amd.render import EpisodeRenderer
    rec, f = recorded(name)
    zoom, ra = RECORDED[name][6:]
    assert ("explored" in f) == (name != "recorded-reward-food")
    assert f["phero"].max() > 1 and f["food"].max() > 0
    ren = EpisodeRenderer(rec, zoom=zoom, ant_radius=ra)  # phero_max_val: the configuration's 255
    assert ren.phero_max_val == 255.0
    img = compare(name, ren, f, 0, 3, 63, ra)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 8  # a picture, not a flat field
    compare(name + "-first-1", ren, f, 1, 1, 63, ra)


def test_defaults_and_refusals_of_the_class():
    from antsrl_amd import _lib
    from antsrl_amd.render import ALL, MAX_ZOOM, EpisodeRenderer
    rec, f = recorded("recorded-default")
    ren = EpisodeRenderer(rec)
    assert (ren.zoom, ren.view, ren.ant_radius, ren.phero_max_val) == (MAX_ZOOM, ALL, MAX_ZOOM // 2, 255.0)  # 900 // 64 = 14 -> 8
    assert tuple(ren.render(2, 1).shape) == (1, 2, 64 * 8, 64 * 8, 3)
    for kw, word in ((dict(zoom=MAX_ZOOM + 1), "zoom"), (dict(zoom=0), "zoom"), (dict(view=64), "view_mask"),
                     (dict(ant_radius=-1), "ant_radius"), (dict(phero_max_val=0.0), "phero_max_val")):
        with pytest.raises(_lib.AntsrlError, match=word):
            EpisodeRenderer(rec, **kw)
    for first, count in ((0, 4), (3, 1), (-1, 1), (0, 0)):
        with pytest.raises(_lib.AntsrlError, match="recorded"):
            ren.render(first, count)
