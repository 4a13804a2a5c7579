"""tests/render_ref.py's colour layer against the reference's own mix_alpha, byte for byte:
tests/golden/contract/render_layer_ref.npz (tests/golden/make_render_golden.py) holds what the viewer's chain gave for a
few small planes.  And the fixture can tell: five wrong restatements of the chain (float32 arithmetic, rounding instead
of truncation, the food behind the pheromones, colour * (a * (1 - A)), one food maximum for all frames) each differ
from it on at least one case.  Host only."""
import os

import numpy as np
import pytest

import render_ref as RR

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contract", "render_layer_ref.npz")
VARIANTS = ("float32", "rounding", "food-last", "association", "global-food-max")


@pytest.fixture(scope="module")
def golden():
    z = np.load(PATH)
    cases = {}
    for name in z["names"].tolist():
        cases[name] = dict(food=z[name + ".food"], phero=z[name + ".phero"], max_val=float(z[name + ".max_val"]),
                           explored=z[name + ".explored"] if name + ".explored" in z.files else None,
                           rgb=z[name + ".rgb"], alpha8=z[name + ".alpha8"])
    return dict(cases=cases, colours=[tuple(int(v) for v in c) for c in z["colours"]], food_color=tuple(z["food_color"].tolist()),
                explored_color=tuple(z["explored_color"].tolist()))


def test_the_fixture_holds_the_cases_the_issue_names(golden):
    c = golden["cases"]
    assert sorted(c) == ["probe_c1_nomap", "small_c1_map", "small_c3_nomap", "wide_c1_nomap", "wide_c3_map"]
    assert {v["food"].shape[1:] for v in c.values()} == {(13, 15), (48, 80)}
    assert {v["phero"].shape[1] for v in c.values()} == {1, 3}
    assert {v["explored"] is None for v in c.values()} == {True, False}
    assert any((v["food"].reshape(len(v["food"]), -1).max(axis=1) == 0).any() for v in c.values())  # an all-zero food plane
    assert any((v["food"] == 255).all(axis=(1, 2)).any() and (v["phero"] == 255).any() for v in c.values())
    assert {255.0, 40.0} <= {v["max_val"] for v in c.values()}
    assert golden["food_color"] == RR.FOOD_COLOR and golden["explored_color"] == RR.EXPLORED_COLOR
    assert os.path.getsize(PATH) < 256 * 1024


def test_render_ref_equals_the_references_mix_alpha_chain(golden):
    for name, c in golden["cases"].items():
        for k in range(len(c["food"])):
            got = RR.colour_layer(c["food"][k], c["phero"][k], None if c["explored"] is None else c["explored"][k],
                                  golden["colours"], c["max_val"])
            assert got.dtype == np.uint8
            assert np.array_equal(got[:, :, :3], c["rgb"][k]), (name, k)
            assert np.array_equal(got[:, :, 3], c["alpha8"][k]), (name, k)


def wrong_layer(variant, food, phero, explored, colours, max_val, food_max):
    """The chain with ONE thing wrong (or, with variant None, nothing: then it is render_ref's)."""
    ft = np.float32 if variant == "float32" else np.float64
    one, eps, eps_food = ft(1), ft(0.001), ft(0.0001)

    def mix(rgb, alpha, colour, a):
        fill = np.array(colour).astype(ft)[None, None, :]
        a3, al3 = a[:, :, None], alpha[:, :, None]
        m = alpha + a * (one - alpha)
        add = fill * (a3 * (one - al3)) if variant == "association" else (fill * a3) * (one - al3)
        v = (rgb.astype(ft) * al3 + add) / (m[:, :, None] + eps)
        return (np.rint(v) if variant == "rounding" else v).astype(np.uint8), m
    rgb, alpha = np.full(food.shape + (3,), 255, dtype=np.uint8), np.zeros(food.shape, dtype=ft)
    layers = [(RR.FOOD_COLOR, food.astype(ft) / (ft(food_max) + eps_food) * ft(0.3))]
    layers += [(colours[k], (phero[k].astype(ft) / (ft(max_val) + eps_food)) * ft(0.6)) for k in range(len(phero))]
    if variant == "food-last":
        layers = layers[1:] + layers[:1]
    if explored is not None:
        layers.append((RR.EXPLORED_COLOR, (explored != 0).astype(ft) / one * ft(0.3)))
    for colour, a in layers:
        rgb, alpha = mix(rgb, alpha, colour, a)
    return np.concatenate([rgb, (alpha * ft(255)).astype(np.uint8)[:, :, None]], axis=2)


@pytest.mark.parametrize("variant", (None,) + VARIANTS)
def test_the_fixture_tells_each_wrong_variant_apart(golden, variant):
    differing = []
    for name, c in golden["cases"].items():
        for k in range(len(c["food"])):
            food_max = c["food"].max() if variant == "global-food-max" else c["food"][k].max()
            got = wrong_layer(variant, c["food"][k], c["phero"][k], None if c["explored"] is None else c["explored"][k],
                              golden["colours"], c["max_val"], food_max)
            if not (np.array_equal(got[:, :, :3], c["rgb"][k]) and np.array_equal(got[:, :, 3], c["alpha8"][k])):
                differing.append((name, k))
    if variant is None:
        assert not differing, differing  # the harness itself is right: only the named change makes a variant differ
    else:
        assert differing, "the fixture cannot tell the %s variant from the reference" % variant


def test_view_bits_skip_layers_entirely(golden):
    c = golden["cases"]["small_c1_map"]
    food, phero, expl = c["food"][0], c["phero"][0], c["explored"][0]
    none = RR.colour_layer(food, phero, expl, golden["colours"], 255.0, view=RR.VIEW_ALL & ~(RR.VIEW_FOOD | RR.VIEW_PHERO | RR.VIEW_EXPLORED))
    assert (none[:, :, :3] == 255).all() and (none[:, :, 3] == 0).all()
    only_food = RR.colour_layer(food, phero, expl, golden["colours"], 255.0, view=RR.VIEW_FOOD)
    want = RR.colour_layer(food, phero[:0], None, golden["colours"], 255.0)
    assert np.array_equal(only_food, want)
