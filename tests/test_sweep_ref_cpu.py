"""sweep_ref on the host: the reference is the oracle's, the plan is safe, the cases are sharp.

  reference  sweep64 equals oracle.oracle.Oracle's grid after step + update with ants that deposit nothing, on every case
             and field: bit for bit where the filter is a single tap (the reference's own DIFFUSE_FACTOR = 0 form, one
             product per cell), within the 1e-12 of test_oracle_golden.py under a patched filter (the order of a
             float64 sum of up to 49 terms is the compiler's).  The action that deposits nothing: pheromone action 0
             (ants.py:89-96 sets both activations to 0; antsrl_oracle.c env_step) where there are two channels, and no
             pheromone action at all elsewhere (activate_pheromone hard-codes two channels; the activation stays at the
             0 of Ants.__init__, ants.py:32).  add_pheromones then adds 0.0 to the ants' cells (pheromone.py:39).
  safe       sweep_decomposed without a defect equals sweep64 bit for bit: a (strip, segment) pair needs nothing but
             its own halo columns and overlap rows.
  sharp      every defect of sweep_ref.DEFECTS, on every case of every kernel it applies to whose plan has the seam it
             sits at (sweep_ref.exposed), fails helpers.phero_close on the dense field.  Two exceptions by arithmetic:
             the two tap defects may be caught on any of the four fields (they are caught on dense as well, asserted
             for information only by the printed line), and cut_applied_before_sum is the identity on a field without a
             value below the cut — equal bits on dense are asserted, and it must fail on near_cut.
  inputs     the cases run over three updates have no reference cell inside the comparator's cut band at any update.
  plan       sweep_plan against a table written by hand from the launcher's comments.
"""
import numpy as np
import pytest

import helpers
import sweep_ref as S
from antsrl_amd import config as cm
from oracle.oracle import Oracle


def _case_inputs(case, field):
    cfg = S.make_case_cfg(case)
    init = S.make_init(case, cfg, field)
    return cfg, init, S.sweep_plan(cfg)


def no_deposit_actions(cfg):
    """(rotation, pheromone action) with which no ant deposits (module docstring)."""
    rot = np.zeros((cfg.n_envs, cfg.n_ants), np.int8)
    return rot, (np.zeros((cfg.n_envs, cfg.n_ants), np.int8) if cfg.n_phero == 2 else None)


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_sweep64_is_the_oracles_update_and_the_plan_is_safe(case):
    for field in S.FIELDS:
        if case.get("huge") and field != "dense":
            continue  # (4.2 M cells: one field for the one property that needs the size, the grid-stride loop's second pass)
        cfg, init, plan = _case_inputs(case, field)
        ref = S.reference(cfg, init)
        orc = Oracle(cfg, init, n_threads=4)
        orc.step(*no_deposit_actions(cfg), want_obs=False)
        assert not orc.activation.any()
        orc.update(None)
        if plan["R"] == 0:
            np.testing.assert_array_equal(orc.phero, ref, err_msg="%s %s" % (case["name"], field))
        else:
            np.testing.assert_allclose(orc.phero, ref, rtol=1e-12, atol=1e-300, err_msg="%s %s" % (case["name"], field))
            np.testing.assert_array_equal(orc.phero == 0, ref == 0)
        dec = S.sweep_decomposed(init["phero"], init["walls"], S.cfg_filter(cfg), cfg.phero_threshold, S.cfg_max_val(cfg), plan)
        np.testing.assert_array_equal(dec, ref, err_msg="%s %s: the plan's pairs do not add up to the sweep" % (case["name"], field))
        assert not np.signbit(dec).any()
        if field == "dense":
            flat = init["phero"].reshape(-1)
            assert flat.min() > 1.0 and flat.max() <= (255.0 if case["max_val"] is None else case["max_val"])
            assert np.unique(flat).size == flat.size, "dense: all values distinct"
        elif field == "near_cut":
            # (the share that is cut to 0 shrinks with the filter's width: 60 % at radius 0, 2 % at radius 3)
            assert ((ref == 0) & (init["phero"] * (init["walls"][:, None] == 0) > 0)).any() and (ref != 0).any()
        elif field == "blocks":
            for e in range(cfg.n_envs):  # both colours of the checkerboard, so every seam has the zero tile on either side
                z = init["phero"][e] == 0
                assert z.any() and (~z).any()
            if cfg.n_envs >= 2:
                assert ((init["phero"][0] == 0) != (init["phero"][1] == 0)).all()
        else:
            assert (init["phero"] == S.IMPULSE).sum() >= 4 * cfg.n_envs * cfg.n_phero


def test_walls_and_impulses_sit_at_the_seams():
    """Per kernel: environment 0 walls every seam-adjacent cell and environment 1 none; the impulses of the channels and
    environments together stand on both sides of every seam and in every corner; one grid at least has a cell count
    that is no multiple of 32 (a partial last bitmap word, environment e + 1's words not where e's cells end)."""
    ragged_words = set()
    for case in S.CASES:
        if case.get("huge"):
            continue
        cfg, init, plan = _case_inputs(case, "impulses")
        if (cfg.w * cfg.h) % 32:
            ragged_words.add(case["kernel"])
        if plan["R"] == 0:
            continue
        xs = [x for x in S._seams(cfg.w, plan["seg_rows"]) if x not in (0, cfg.w - 1)]
        ys = [y for y in S._seams(cfg.h, plan["strip_w"]) if y not in (0, cfg.h - 1)]
        assert init["walls"][0][xs, :].all() and init["walls"][0][:, ys].all(), case["name"]
        assert not init["walls"][1][xs, :].any() and not init["walls"][1][:, ys].any(), case["name"]
        hit = (init["phero"] == S.IMPULSE).any(axis=(0, 1))
        assert hit[0, 0] and hit[0, -1] and hit[-1, 0] and hit[-1, -1], case["name"]
        assert hit[xs, :].any(axis=1).all() and hit[:, ys].any(axis=0).all(), case["name"]
        R = plan["R"]
        for e in range(cfg.n_envs):
            for c in range(cfg.n_phero):
                px, py = np.nonzero(init["phero"][e, c])
                d = np.maximum(np.abs(px[:, None] - px[None, :]), np.abs(py[:, None] - py[None, :]))
                d[np.arange(len(px)), np.arange(len(px))] = 99
                assert d.min() >= 2 * R + 1, case["name"]
    assert ragged_words >= set(S.FAMILIES) - {"k_sweep0<4>"}, set(S.FAMILIES) - ragged_words  # (C = 4 at 256 or 1024 float4: 16 x 16, 32 x 32)


# (the one grid past the scalar kernel's cap of 16384 workgroups has one channel: its loop is the same code at C = 2, 3)
_PAIRS = [(k, d) for k in S.FAMILIES for d in S.APPLIES[next(c for c in S.CASES if c["kernel"] == k)["family"]]
          if not (d == "grid_stride_single_pass" and k != "k_sweep0_scalar<1>")]


@pytest.mark.parametrize("kernel,defect", _PAIRS, ids=["%s-%s" % p for p in _PAIRS])
def test_every_defect_is_caught(kernel, defect, capsys):
    caught = []
    for case in (c for c in S.CASES if c["kernel"] == kernel):
        plan = S.sweep_plan(S.make_case_cfg(case))
        if not S.exposed(defect, plan):
            continue
        fields = ("dense",) if not defect.startswith("tap_") else S.FIELDS
        if defect == "cut_applied_before_sum":
            fields = ("dense", "near_cut")
        by = None
        for field in fields:
            cfg, init, plan = _case_inputs(case, field)
            ref = S.reference(cfg, init)
            bad = S.sweep_decomposed(init["phero"], init["walls"], S.cfg_filter(cfg), cfg.phero_threshold, S.cfg_max_val(cfg),
                                     plan, defect=defect)
            if defect == "cut_applied_before_sum" and field == "dense":
                np.testing.assert_array_equal(bad, ref)  # no value below the cut: the identity
                continue
            nbad = int((~helpers.phero_close(bad, ref, threshold=cfg.phero_threshold)).sum())
            if nbad:
                by = (field, nbad)
                break
        assert by is not None, "%s: %s passes the comparator on %s — a gap in CASES" % (case["name"], defect, fields)
        caught.append((case["name"], by[0], by[1]))
    assert caught, "%s: no case of %s has the seam it sits at" % (defect, kernel)
    with capsys.disabled():
        print("\nCAUGHT %-34s %-24s %d case(s), each on field %s; first: %s (%d cells off)" % (
            defect, kernel, len(caught), "/".join(sorted({c[1] for c in caught})), caught[0][0], caught[0][2]))


_MULTI = [c for c in S.CASES if c.get("multi")]


@pytest.mark.parametrize("case", _MULTI, ids=[c["name"].replace(" ", "_") for c in _MULTI])
def test_multi_step_inputs_stay_out_of_the_cut_band(case):
    cfg = S.make_case_cfg(case)
    for field in ("dense", "near_cut"):
        nudged, init, refs = S.multi_inputs(case, field)
        assert len(refs) == S.MULTI_STEPS
        bw = helpers.CUT_BAND_RTOL * cfg.phero_threshold
        for t, r in enumerate(refs):
            assert not (np.abs(r - cfg.phero_threshold) <= bw).any(), "%s %s update %d" % (case["name"], field, t)
        assert (refs[-1] != 0).any(), "the field has died out before the last update"
        assert nudged <= 16, "the mended field is still the case's field"
        if field == "dense":
            flat = init["phero"].reshape(-1)
            assert flat.min() > 1.0 and np.unique(flat).size == flat.size


@pytest.mark.parametrize("case", _MULTI, ids=[c["name"].replace(" ", "_") for c in _MULTI])
def test_deposit_inputs_deposit_and_stay_out_of_the_cut_band(case):
    cfg, init, act, steps = S.deposit_inputs(case)
    orc = Oracle(cfg, init, n_threads=4)
    if act is not None:
        orc.set_activation(act)
    before = S.reference(cfg, init)
    for t, (rot, ph, jit) in enumerate(steps):
        orc.step(rot, ph, want_obs=False)
        orc.update(jit)
        assert orc.activation.any()
        assert not S.in_cut_band(orc.phero, cfg.phero_threshold).any(), "%s update %d" % (case["name"], t + 1)
        if t == 0:
            assert (orc.phero != before).sum() >= cfg.n_envs * 8, "the ants deposit"


def test_sweep_plan_against_the_launchers_comments():
    """Six shapes by hand.  c3 + 3 x 3 diffusion (256 x 256, two channels: 'H = 256: two strips', 16 rows per segment);
    c4 (512 x 512, radius-3 Gaussian, two columns per lane: 32 rows, strips of 128 - 4 SEP2_HL = 112 columns); the same
    filter at odd H (one column per lane: 64 rows, strips of 58); C = 3 with a general radius-2 filter (32 rows, strips
    of 60); the shipped radius-0 filter on c3's grid (32768 float4 per environment, blocks of 1024); a 41 x 41 grid of
    one channel (1681 floats per environment: the scalar kernel)."""
    ax = np.arange(-3, 4)
    g = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / 4.5)
    g = g / g.sum() * 0.999
    table = [
        (dict(C=2, W=256, H=256, filt=cm.diffuse_filter(0.02, 0.001)), dict(kernel="k_sweep_r1x2", seg_rows=16, nsegs=16, strip_w=128, nstrips=2)),
        (dict(C=2, W=512, H=512, filt=g), dict(kernel="k_sweep_sep2<3>", seg_rows=32, nsegs=16, strip_w=112, nstrips=5)),
        (dict(C=2, W=100, H=41, filt=g), dict(kernel="k_sweep_march<2,3,1>", seg_rows=64, nsegs=2, strip_w=58, nstrips=1)),
        (dict(C=3, W=70, H=122, filt=S.stencil_filter(2, False, 20)), dict(kernel="k_sweep_march<3,2,0>", seg_rows=32, nsegs=3, strip_w=60, nstrips=3)),
        (dict(C=2, W=256, H=256, filt=np.array([[0.999]])), dict(kernel="k_sweep0<2>", float4_per_env=32768, block=1024, nblocks=32)),
        (dict(C=1, W=41, H=41, filt=np.array([[0.999]])), dict(kernel="k_sweep0_scalar<1>", n=3 * 1681, blocks=20, passes=1)),
    ]
    for case, want in table:
        plan = S.sweep_plan(S.make_case_cfg(dict(case, E=3, max_val=255.0)))
        assert {k: plan[k] for k in want} == want, (case, plan)
