#!/usr/bin/env python3
"""Generates tests/golden/contract/render_layer_ref.npz by RUNNING THE REFERENCE'S OWN mix_alpha (gui/visualize.py:23-26) —
build container only (the reference lives at /root/reference there and never travels).

The viewer's colour layer is a chain of mix_alpha calls over the snapshot's objects in their order (food, the
pheromones, the RL visualisation's heatmap: visualize.py:220-244), each with the alpha expression the viewer writes
inline.  This script runs that chain, with those expressions, on a few small uint8 planes and stores the inputs and the
bytes that came out: color_repr_img and (color_repr_alpha * 255).astype(np.uint8) (visualize.py:267).  Nothing of the
reference's source is stored.

gui/visualize.py imports pygame at its top; pygame is not installed and mix_alpha does not use it, so an EMPTY stand-in
module is registered under that name for the import and removed again (and `noise`, as in make_contract_golden.py).

Cases (name: W x H, C pheromones, heatmap, max_val; n frames each):
  small_c1_map      13 x 15, 1, yes, 255   dense random; a frame whose food plane is all zero; a frame of all 255
  small_c3_nomap    13 x 15, 3, no,  255   dense random; a frame of all zero
  wide_c3_map       48 x 80, 3, yes, 40    pheromone in 0..40 (what a max_val of 40 clips to), food maxima 255 and 9
  wide_c1_nomap     48 x 80, 1, no,  255   sparse planes, food maxima 200 and 3
  probe_c1_nomap    13 x 15, 1, no,  PROBE_MAX_VAL   dense random, with the cell (0, 0) of frame 0 planted (see below)

Rounding the chain's products in another association (colour * (a * (1 - A)) for (colour * a) * (1 - A)) moves a value
by an ulp, which changes a byte only where the value lies within an ulp of an integer: no random plane has such a cell.
max_val is a float64, though, and the value moves with it: PROBE_MAX_VAL was found by bisecting max_val for the point
where the red channel of a cell with food 37 (of a maximum of 255) and pheromone 7 crosses an integer, then walking the
neighbouring doubles for one at which the two associations fall on different sides.  tests/test_render_ref_cpu.py
checks that the fixture tells that variant apart.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.modules.setdefault("noise", types.ModuleType("noise"))  # utils.py:2
_had = sys.modules.get("pygame")
sys.modules["pygame"] = types.ModuleType("pygame")           # for this import only
from gui.visualize import FOOD_COLOR, PERCEPTIVE_FIELD_COLOR, mix_alpha  # noqa: E402
if _had is None:
    del sys.modules["pygame"]
else:
    sys.modules["pygame"] = _had

AX = np.newaxis
PROBE_MAX_VAL, PROBE_FOOD, PROBE_PHERO = 59.17310556547085, 37, 7
COLOURS = ((255, 64, 0), (64, 64, 255), (100, 255, 100))


def viewer_layer(food, phero, heatmap, max_val):
    """One frame through the viewer's chain: the fills of setup_environment (:73-74, :88), the alphas of :222, :231, :240."""
    w, h = food.shape
    fill = lambda c: np.array(c)[AX, AX, :].repeat(w, axis=0).repeat(h, axis=1)  # noqa: E731
    img = np.zeros((w, h, 3), dtype=np.uint8)
    img[:, :, :] = 255
    alpha = np.zeros((w, h))
    img, alpha = mix_alpha(img, alpha, fill(FOOD_COLOR), food / (np.max(food) + 0.0001) * 0.3)
    for k in range(len(phero)):
        img, alpha = mix_alpha(img, alpha, fill(COLOURS[k]), (phero[k] / (max_val + 0.0001)) * 0.6)
    if heatmap is not None:
        img, alpha = mix_alpha(img, alpha, fill(PERCEPTIVE_FIELD_COLOR), (heatmap / np.max(heatmap)) * 0.3)
    return img, (alpha * 255).astype(np.uint8)


def planes(rng, n, w, h, c, heatmap, phero_top, food_tops, density):
    keep = lambda: rng.random((n, w, h)) < density  # noqa: E731
    food = np.stack([rng.integers(0, t + 1, (w, h)) for t in food_tops]).astype(np.uint8) * keep()
    for k, t in enumerate(food_tops):
        food[k, rng.integers(w), rng.integers(h)] = t  # the frame's maximum is what the case names
    phero = (rng.integers(0, phero_top + 1, (n, c, w, h)) * np.stack([keep() for _ in range(c)], axis=1)).astype(np.uint8)
    expl = (rng.random((n, w, h)) < 0.5) if heatmap else None
    if heatmap:
        expl[:, 0, 0] = True  # (an all-false map is 0 / 0 in the viewer)
    return food.astype(np.uint8), phero, expl


def main():
    rng = np.random.default_rng(20240607)
    cases = {}
    f, p, e = planes(rng, 3, 13, 15, 1, True, 255, (255, 0, 255), 1.0)
    f[1] = 0
    f[2], p[2] = 255, 255
    cases["small_c1_map"] = (f, p, e, 255.0)
    f, p, e = planes(rng, 2, 13, 15, 3, False, 255, (255, 0), 1.0)
    f[1], p[1] = 0, 0
    cases["small_c3_nomap"] = (f, p, e, 255.0)
    cases["wide_c3_map"] = planes(rng, 2, 48, 80, 3, True, 40, (255, 9), 1.0) + (40.0,)
    cases["wide_c1_nomap"] = planes(rng, 2, 48, 80, 1, False, 255, (200, 3), 0.15) + (255.0,)
    f, p, e = planes(rng, 2, 13, 15, 1, False, 59, (255, 31), 1.0)
    f[0, 0, 0], p[0, 0, 0, 0] = PROBE_FOOD, PROBE_PHERO
    f[0, 1, 1] = 255
    cases["probe_c1_nomap"] = (f, p, e, PROBE_MAX_VAL)
    out = {"names": np.array(sorted(cases)), "colours": np.array(COLOURS, dtype=np.uint8),
           "food_color": np.array(FOOD_COLOR, dtype=np.uint8), "explored_color": np.array(PERCEPTIVE_FIELD_COLOR, dtype=np.uint8)}
    for name, (food, phero, expl, max_val) in cases.items():
        res = [viewer_layer(food[k], phero[k], None if expl is None else expl[k], max_val) for k in range(len(food))]
        out[name + ".food"], out[name + ".phero"], out[name + ".max_val"] = food, phero, np.float64(max_val)
        if expl is not None:
            out[name + ".explored"] = expl.astype(np.uint8)
        out[name + ".rgb"] = np.stack([r[0] for r in res])
        out[name + ".alpha8"] = np.stack([r[1] for r in res])
        assert out[name + ".rgb"].dtype == np.uint8 and out[name + ".alpha8"].dtype == np.uint8
        assert int(food.max(axis=(1, 2)).min()) != int(food.max()), name  # the frames' food maxima differ
    path = os.path.join(HERE, "contract", "render_layer_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
