"""What the device tests of the memory agent's training step rest on, shown on the CPU.

The exact cases (memory_train_cases.EXACT) are exact: in float64 without any rounding, (a) every value at a bf16
rounding point of the contract is bf16-representable, (b) every product sum and row sum satisfies
sum |terms| < 2^24 x (the lowest set bit of its terms), so every partial sum in every order is an integer multiple of that
bit below 2^24 of it and fp32 holds it exactly, (c) every 32 x 32 tile of every trained weight gradient holds a nonzero,
and so do its last real row and last real column.  (c) is asserted at every case but the one of a single row: one row's
weight gradient is one outer product, a head's dOut has one nonzero and a hidden layer's a handful (the columns of W
that the taken action owns, thinned by three ReLU masks), so no input covers every tile; that case is there for the
row tile of one row, its coverage is recorded, and it is asserted that each tensor's gradient is not all zero.

The layouts restated in memory_train_ref give antsrl_memtrain_sizes' byte counts at every case and over a sweep.

The stage bound (memory_train_ref.stage_outputs) is safe and sharp at every stage case: the fp32 restatement of each
launch, in a summation order of its own, stays inside it (its share is printed), and each of twelve planted defects
leaves it at every case it can touch.  Where a defect is the identity on a case by arithmetic, the condition is stated
below and equality is asserted instead; no case is skipped."""
import ctypes as C

import pytest
import torch

import memory_train_cases as K
import memory_train_ref as R

DEFECTS = {  # defect -> the launches it is planted in
    "last_column_dropped": ("fwd0",),
    "bias_on_padding": R.STAGES[:7],
    "mask_ge_0": ("bwd3", "bwd4", "bwd5"),
    "mask_from_wrong_layer": ("bwd3", "bwd4", "bwd5"),
    "w_for_wt": R.STAGES[8:14],
    "dg_second_segment_omitted": ("bwd2",),
    "residual_dropped": ("fwd3",),
    "dones_ignored": ("td",),
    "scale_2_over_B": ("td",),
    "tail_rows_dropped": ("wgrad",),
    "db_first_tile_only": ("wgrad",),
    "stale_pack": R.STAGES[:7] + R.STAGES[8:14],
}


def _bf16_ok(t):
    return bool((t.float().to(torch.bfloat16).double() == t).all())


def _coverage(c, grads):
    """(tiles without a nonzero, last rows / columns without one, nonzero share by tensor) over the weight gradients."""
    bare, edges, share = [], [], {}
    for n in R.TRAINED:
        g = grads[n + ".weight"]
        share[n + ".weight"] = float((g != 0).double().mean())
        share[n + ".bias"] = float((grads[n + ".bias"] != 0).double().mean())
        for o0 in range(0, g.shape[0], 32):
            for i0 in range(0, g.shape[1], 32):
                if not bool(g[o0:o0 + 32, i0:i0 + 32].any()):
                    bare.append((n, o0, i0))
        if not bool(g[-1].any()):
            edges.append((n, "last row"))
        if not bool(g[:, -1].any()):
            edges.append((n, "last column"))
    return bare, edges, share


@pytest.mark.parametrize("case", K.EXACT, ids=K.EXACT_IDS)
def test_exact_cases_are_exact(case):
    assert case["n_rot"] == 32 and case["n_ph"] == 32 and case["B"] & (case["B"] - 1) == 0 and case["discount"] == 0.5
    inp = K.exact_inputs(case)
    for sd in (inp["sd"], inp["target"]):
        for n in R.TRAINED:
            w = sd[n + ".weight"]
            assert bool(((w == 0) | (w.abs() == 1)).all()) and bool(w.abs().sum(0).min() >= 1), n  # no column all zero
    t = K.exact_trace(case, inp)
    for what, v in t["rounded"]:                                   # (a)
        assert _bf16_ok(v), (what, float(v.abs().max()))
    for what, total, low in t["sums"]:                             # (b)
        assert float(total.max()) < 2.0 ** 24 * low, (what, float(total.max()), low)
    f = K.flat(t["grads"])
    assert bool((f.float().double() == f).all()) and float(torch.as_tensor(t["loss"]).float()) == float(t["loss"])
    bare, edges, share = _coverage(case, t["grads"])               # (c)
    print("EXACT-COVERAGE %s %s" % (case["name"], {k: round(v, 4) for k, v in share.items()}))
    if case["B"] > 1:
        assert not bare and not edges, (bare, edges)
    else:
        print("  one row: %d tiles and %d edges without a nonzero" % (len(bare), len(edges)))
        assert all(bool(t["grads"][n + s].any()) for n in R.TRAINED[3:] for s in (".weight", ".bias"))


def test_inexact_batch_sizes_fail_the_premise():
    """The premise has teeth: where 2 / (B n) is no power of two, dOut is not bf16-representable."""
    for B in (264, 513, 4097):
        c = dict(K.EXACT[1], B=B, name="inexact")
        t = K.exact_trace(c, K.exact_inputs(c))
        assert not all(_bf16_ok(v) for _, v in t["rounded"]), B


@pytest.fixture(scope="module")
def lib():
    from antsrl_amd import _lib
    from antsrl_amd import build as buildmod
    buildmod.build_hip()
    return _lib.load()


def _sizes(lib, F, power, mem, n_rot, n_ph, B):
    from antsrl_amd import _lib
    s = _lib.AntsMemNetShape(F, 2, mem, 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power), n_rot, n_ph)
    out = [C.c_size_t() for _ in range(4)]
    assert lib.antsrl_memtrain_sizes(C.byref(s), B, *[C.byref(o) for o in out]) == 0
    return [o.value for o in out]


def test_the_layout_restatement_gives_the_library_sizes(lib):
    shapes = [K.dims(c) + (c["B"],) for c in K.EXACT + K.STAGE]
    for F in (1, 31, 294, 990):
        for power, mem in ((4, 1), (5, 20), (4, 32)):
            for B in (1, 32, 33, 255, 256, 257, 8192, 8193, 16384, 16385, 16416, 16417, 65536, 1 << 24):
                shapes.append((F, power, mem, 1 + (F + B) % 32, 1 + (F * B) % 32, B))
    for F, power, mem, n_rot, n_ph, B in shapes:
        W = R.work_layout(F, power, mem, n_rot, n_ph, B)
        L = W["L"]
        assert [L["params_floats"], L["trained_floats"], L["bytes"], W["bytes"]] == _sizes(lib, F, power, mem, n_rot, n_ph, B), \
            (F, power, mem, n_rot, n_ph, B)


def _problem(case):
    inp = K.stage_inputs(case)
    return R.problem(inp["sd"], inp["target"], inp["arrays"], inp["idx"], case["B"], case["discount"], K.dims(case),
                     stale=inp["stale"])


def _same(a, b):
    return all(torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])) for k in a)


def _identity(defect, case, P):
    """The cases on which a defect is the identity, by arithmetic (None: it must leave the bound)."""
    L = P["L"]
    if defect == "bias_on_padding":      # no layer has a padded column: D, n_rot and n_ph are all multiples of 32
        return all(L["out"][l] % 32 == 0 for l in range(9))
    if defect == "dones_ignored":        # (1 - done) multiplies discount * max q': no row done (dones none, B = 1), or discount 0
        return not bool(P["dn"].any()) or case["discount"] == 0.0
    if defect == "scale_2_over_B":       # n = 1: the same number
        return case["n_rot"] == 1 and case["n_ph"] == 1
    if defect == "tail_rows_dropped":    # no partial row tile
        return case["B"] % 32 == 0
    return False


@pytest.mark.parametrize("case", K.STAGE, ids=K.STAGE_IDS)
def test_the_stage_bound_is_safe_and_sharp(case):
    P = _problem(case)
    img = R.simulate(P)
    shares = {s: R.check_stage(s, img, P) for s in R.STAGES}
    print("STAGE-CPU-SHARE %s %s" % (case["name"], {s: round(v, 4) for s, v in shares.items()}))
    assert max(shares.values()) <= 1.0, shares
    mildest = {}
    for defect, stages in DEFECTS.items():
        worst, same = 0.0, True
        for s in stages:
            got = R.stage_outputs(s, img, P, torch.float32, defect)[0]
            same = same and _same(got, {k: img[k] for k in got})
            worst = max(worst, R.check_stage(s, img, P, got))
            if worst > 1.0 and not _identity(defect, case, P):
                break
        if _identity(defect, case, P):
            assert same, (defect, "expected the identity")
            continue
        mildest[defect] = worst
        assert worst > 1.0, (case["name"], defect, worst)
    print("STAGE-CPU-DEFECT %s %s" % (case["name"], {d: (round(v, 1) if v < 1e9 else "inf") for d, v in mildest.items()}))
