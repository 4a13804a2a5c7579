"""The cases of population_stage_cases.py are what they are for, certified on the references alone (no native code):
enough rows of every acting case are clear for the comparison with float64 to mean something, a wrong reading of a member's
net, layer3 or rows would show on a clear row, a member trained with its neighbour's discount or step size leaves the
bound, and every regime the cases are named for is reached under the restated launch rules.  Conditions, not measurements."""
import copy

import numpy as np
import pytest
import torch

import linear_train_cases as K
import linear_train_ref as L
import population_stage_cases as S

BOUND_HEADS = 1e-4  # test_gpu_linear_agent.py's: |p - p_ref| in units of one step of lr


# ---- linear_train_cases.inputs(member=)
@pytest.mark.parametrize("name", ["width-F9-B33", "seam-F294-B512", "clamp-actions"])
def test_member_0_is_the_case_as_it_stands(name):
    case = next(c for c in K.CASES if c["name"] == name)
    assert K.input_seed(case) == K.input_seed(case, 0) == 1000 * case["F"] + case["B"] + 7 * case["N"]  # the seed it always had

    def flat(inp):
        out = list(inp["sd"].values()) + list(inp["target"]) + list(inp["arrays"]) + [inp["idx"]]
        return out + ([inp["raw"]] if inp["raw"] is not None else [])
    plain, zero, one = flat(K.inputs(case)), flat(K.inputs(case, member=0)), flat(K.inputs(case, member=1))
    assert len(plain) == len(zero) == len(one)
    for a, b, c in zip(plain, zero, one):
        assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes()
        assert a.shape == c.shape and not torch.equal(a, c), "member 1 differs in every tensor"


# ---- acting: the shares of clear rows
@pytest.mark.parametrize("name", S.ACTING_IDS)
def test_enough_rows_are_clear(name):
    c = S.acting_case(name)
    share = c["clear"].double().mean(dim=1)  # [P, 2]
    both = (c["clear"][:, :, 0] & c["clear"][:, :, 1]).double().mean(dim=1)
    print("\nCERTIFIED %s: least share of clear rows over the members: rotation %.3f, pheromone %.3f, both heads %.3f"
          % (name, float(share[:, 0].min()), float(share[:, 1].min()), float(both.min())))
    assert bool((share >= S.CLEAR_SHARE).all()), share
    if c["Mm"] == 1:
        assert bool(c["clear"].all()), "the one row must be clear"


def _changes(c, p, rot, ph, heads):
    """Whether the actions (rot, ph) of a wrong reading differ from member p's on a row clear on one of `heads`."""
    clear = c["clear"][p]
    diff = torch.stack([rot != c["rot"][p], ph != c["ph"][p]], 1)
    return bool((diff & clear)[:, list(heads)].any())


# ---- acting: wrong readings would show
@pytest.mark.parametrize("name", S.ACTING_IDS)
def test_wrong_readings_change_a_clear_row(name):
    """Each on the rotation head alone too, which is all the explore net has.  A population of one member has no
    neighbour, and a batch of one row no other tile: A4-one is held by the live layer3 alone (and by bit equality with the
    single policy on the device)."""
    c = S.acting_case(name)
    inp, P, Mm = c["inp"], c["P"], c["Mm"]
    allx, alla = inp["obs"].reshape(P * Mm, -1), inp["ast"].reshape(P * Mm, 2)
    for p in range(P):
        if P > 1:  # the neighbour's net: a wrong stride of the weights, a table entry read for the wrong member
            rot, ph = S.decide(S.acting_forward(inp, p, net=(p + 1) % P)[0])
            assert _changes(c, p, rot, ph, (0,)) and _changes(c, p, rot, ph, (1,)), (p, "neighbour")
        rot, ph = S.decide(S.acting_forward(inp, p, l3="live")[0])  # the live layer3 in place of the target's
        assert torch.equal(rot, c["rot"][p]) and _changes(c, p, rot, ph, (1,)), (p, "live layer3")
        if P * Mm > 1:  # the rows one tile on in the batch (a launch rule off by one tile, a wrong stride of the rows)
            idx = (torch.arange(Mm) + p * Mm + 32) % (P * Mm)
            assert not torch.equal(idx, torch.arange(Mm) + p * Mm)
            rot, ph = S.decide(S.acting_forward(inp, p, rows=(allx[idx], alla[idx]))[0])
            assert _changes(c, p, rot, ph, (0,)) and _changes(c, p, rot, ph, (1,)), (p, "shifted rows")
    # the members' nets all differ, and no target layer3 is the live one
    for k in ("w1", "b1", "w2", "b2", "tw3", "tb3"):
        assert len({inp[k][p].numpy().tobytes() for p in range(P)}) == P, k
    assert not bool((inp["tw3"] == inp["w3"]).all(dim=(1, 2)).any()) and not bool((inp["tb3"] == inp["b3"]).all(dim=1).any())
    # both formats carry the same numbers
    assert torch.equal(inp["obs"].to(torch.bfloat16).float(), inp["obs"])


# ---- acting: the regimes are reached
def test_acting_regimes():
    launch = {n: S.acting_launch(c) for n, c in S.ACTING.items()}
    for n, c in S.ACTING.items():
        Mm, F = c["Em"] * c["N"], c["F"]
        assert S.pol_flat_fits(F) and 1 <= c["P"] <= S.POP_MAX
        for esz in (2, 4):  # the acting alignment rule, both formats
            assert (Mm * F * esz) % 16 == 0, (n, esz)
        assert sorted(r for w in launch[n]["waves"] for r in w) == sorted([32] * (Mm // 32) + ([Mm % 32] if Mm % 32 else []))
    a1, a2, a3, a4, one, a5 = (launch[n] for n in S.ACTING_IDS)
    # A1: F < 16 and odd, one partial k-step, one tile of 8 rows
    assert S.ACTING["A1"]["F"] == 9 and a1["waves"] == [[8], []]
    # A2: a partial last k-step, a whole tile and one of 4 rows in one workgroup
    assert S.ACTING["A2"]["F"] % 16 == 2 and a2["waves"] == [[32], [4]]
    # A3: the opt-in (needed from F = 337 on: 343 is the first 7 x 7 x K beyond it, and odd); two workgroups per member
    assert next(F for F in range(1, 849) if S.pol_flat_lds(F) > S.LDS_PLAIN) == 337
    assert S.LDS_PLAIN < S.pol_flat_lds(343) == 67072 == a3["lds"] and S.ACTING["A3"]["F"] % 2 == 1
    assert a3["blocks"] == 2 and a3["cap"] > 2
    for n in ("A1", "A2", "A5"):
        assert launch[n]["lds"] <= S.LDS_PLAIN, n
    # A4: the widest row the flat form takes, one workgroup per CU; F = 849 does not fit
    assert a4["lds"] == one["lds"] == 163456 <= S.LDS_CU == 163840 and a4["per_cu"] == one["per_cu"] == 1
    assert S.pol_flat_fits(848) and not S.pol_flat_fits(849)
    assert a4["waves"] == [[32], [2]] and one["waves"] == [[1], []]
    # A5: P at its maximum; the cap of 8 workgroups bites where 9 are wanted, so waves loop, and wave 1 meets the 4-row
    # tile 17 behind the full tile 1
    assert S.ACTING["A5"]["P"] == S.POP_MAX and (a5["want"], a5["cap"], a5["blocks"], a5["per_cu"]) == (9, 8, 8, 2)
    assert a5["ntiles"] == 18 and a5["waves"][0] == [32, 32] and a5["waves"][1] == [32, 4] and all(w == [32] for w in a5["waves"][2:])
    assert 64 * 548 * 294 * 4 < 42e6  # the largest allocation of the device tests: A5's float32 observations


# ---- select and record: the regimes are reached
def test_select_and_record_regimes():
    s = S.SELECT
    assert {e for c in s.values() for e in c["eps"]} == {0.0, 0.5, 1.0}
    assert all(len(c["seeds"]) == len(c["eps"]) == c["P"] for c in s.values())
    assert s["S1"]["seeds"][0] == s["S1"]["seeds"][2] and s["S2-P64"]["P"] == S.POP_MAX
    assert s["S3-base-step"]["base"] == 11 and s["S3-base-step"]["step"] == 2 ** 40 + 3 >= 2 ** 32
    assert s["S4-blocks"]["Em"] * s["S4-blocks"]["N"] == 900 > 3 * 256
    for c in s.values():  # a member that explores and one that does not, wherever the epsilons allow both
        rot, ph = S.select_inputs(c)
        r, p, ex = S.select_expected(c, rot, ph)
        ex = ex.reshape(c["P"], c["Em"])
        for m in range(c["P"]):
            assert c["eps"][m] != 0.0 or not ex[m].any()
            assert c["eps"][m] != 1.0 or ex[m].all()
        assert ex.any() and not ex.all()
        keep = np.repeat(~ex.reshape(-1), c["N"]).reshape(rot.shape)
        assert np.array_equal(r[keep], rot[keep]) and np.array_equal(p[keep], ph[keep])
    # two members that share a seed differ through their environment ids
    c = s["S1"]
    assert not np.array_equal(S.select_expected(dict(c, eps=(1.0,) * 3), *S.select_inputs(c))[0][0:2],
                              S.select_expected(dict(c, eps=(1.0,) * 3), *S.select_inputs(c))[0][4:6])

    r1, r2, r3 = (S.RECORD[n] for n in S.RECORD_IDS)
    F = int(np.prod(r1["space"]))
    # R1: odd F and an odd ring: the members' slabs start at different 16-byte phases, and so do the rows inside a slab
    assert F % 2 == 1 and r1["max_len"] % 2 == 1
    assert len({(p * r1["max_len"] * F * 4) % 16 for p in range(r1["P"])}) >= 2
    assert {(row * F * 4) % 16 for row in range(4)} == {0, 4, 8, 12}  # the copy's h: 0 .. 3 elements in front
    Mm = r1["Em"] * r1["N"]
    assert {(a * F * 2) % 8 for a in range(Mm)} >= {0, 2, 4, 6} and {(a * F * 4) % 16 for a in range(Mm)} == {0, 4, 8, 12}
    assert r1["K"] < Mm and r1["base"] != 0 and r1["head"] + r1["K"] > r1["max_len"] > r1["head"]  # sampled; wraps mid-launch
    # R2: K = all > max_len: j0 = 16, and the 50 entries written are no whole number of workgroups
    assert r2["K"] is None and Mm - r2["max_len"] == 16 and r2["max_len"] % 4 != 0
    assert r3["P"] == S.POP_MAX and r3["head"] + r3["K"] > r3["max_len"]
    for c in (r1, r2, r3):
        inp = S.record_inputs(c)
        want, written = S.record_expected(c, inp)
        k = c["Em"] * c["N"] if c["K"] is None else c["K"]
        assert (written.sum(axis=1) == min(k, c["max_len"])).all()
        assert np.isnan(want["states"][~written]).all() and (want["dones"][~written] == S.FILL_DONE).all()
        done = inp["done"].reshape(c["P"], c["Em"])
        assert len(np.unique(inp["done"])) == 2 and (c["Em"] == 1 or (done[:, 0] != done[:, 1]).any())
        # the members differ in what they wrote, the two that share a seed included
        assert len({want["states"][p].tobytes() for p in range(c["P"])}) == c["P"]


# ---- the collect step
def test_collect_step_regimes():
    widths = sorted({c["F"] for c in S.TRAIN.values()})
    assert widths == [9, 50, 294, 1022] and sorted({c["B"] for c in S.TRAIN.values()}) == [1, 33, 264, 512]
    assert [S.lt_lds(F) > S.LDS_PLAIN for F in widths] == [False, False, False, True]  # F = 1022 takes the opt-in
    assert S.lt_lds(608) <= S.LDS_PLAIN < S.lt_lds(609) and S.lt_lds(1022) <= S.LDS_CU
    assert S.TRAIN["P64-F50-B33"]["P"] == S.POP_MAX
    c = S.train_case("P64-F50-B33")
    for p in range(64):  # every member differs from its neighbour in discount and learning rate, 63 from 0 too
        q = (p + 1) % 64
        assert c["discount"][p] != c["discount"][q] and c["lr"][p] != c["lr"][q]
    assert S.train_case("F9-B1")["discount"] == (0.5, 0.99, 0.9) and S.train_case("F9-B1")["lr"] == (1e-3, 1e-4, 3e-3)


@pytest.mark.parametrize("name", S.TRAIN_IDS)
def test_a_neighbours_discount_or_step_size_leaves_the_bound(name):
    c = S.train_case(name)
    P, B = c["P"], c["B"]
    seen = []
    for p in range(P if P <= 3 else 5):  # P = 64: the five hyper-parameter sets once
        q = (p + 1) % P
        inp = S.train_inputs(c, p)
        seen.append(inp)
        assert bool(torch.isnan(inp["ring"][0]).any(dim=1).sum() == c["N"] - len(set(inp["idx"].tolist())))
        assert sorted(inp["idx2"].tolist()) == sorted(inp["idx"].tolist()) and (B == 1 or not torch.equal(inp["idx2"], inp["idx"]))
        host = L.new_state(inp["sd"])
        host["target_w3"], host["target_b3"] = inp["target"]
        batch = K.gathered(inp, B)
        _, g = L.contract_train_step(host, batch, c["discount"][p], update=False)
        bound = L.fp32_sum_bounds(host, batch, c["discount"][p])
        _, g_wrong = L.contract_train_step(host, batch, c["discount"][q], update=False)
        assert L.worst_share(g_wrong, g, bound) > 1.0, (p, "the neighbour's discount stays inside the bound")
        mine, theirs = copy.deepcopy(host), copy.deepcopy(host)
        L.adam(mine, g, c["lr"][p])
        L.adam(theirs, g, c["lr"][q])
        off = max(float((mine["sd"][k] - theirs["sd"][k]).abs().max()) for k in L.TRAINED) / c["lr"][p]
        assert off > BOUND_HEADS, (p, "the neighbour's step size stays inside the bound")
    flat = lambda i: list(i["sd"].values()) + list(i["target"]) + list(i["arrays"]) + ([i["idx"]] if B > 2 else [])  # noqa: E731
    for a, b in zip(seen, seen[1:]):  # the members' inputs differ in every tensor (inputs fixes idx[0] = 0, idx[B - 1] = 1)
        assert not any(torch.equal(x, y) for x, y in zip(flat(a), flat(b)))
