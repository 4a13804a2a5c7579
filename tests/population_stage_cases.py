"""The shapes, seeded inputs and float64 references at which the two populations' kernels are tested stage by stage, off
the fused loop's two shapes ("Held alone at"): one list, shared by the device tests
(test_gpu_population_stages.py) and by the CPU test that certifies the cases are what they are for
(test_population_stage_cases_cpu.py).  CPU only, no native code: torch and numpy from seeded generators.

  acting        ACTING and acting_case(name): per member a net of its own (nn.Linear's init; a target layer3 that is not the
                live one), observations U(-1, 1) on bfloat16 values (so both observation formats carry the same numbers),
                agent states U(0, 5); acting_forward: the net in float64 on the bfloat16-rounded operands, with a bound
                per row and head that is derived, not measured, and the rows that are CLEAR under it.
  select        SELECT: the batches of antsrl_pop_select, with their members' seeds and epsilons.
  record        RECORD, record_inputs and record_expected: the numpy restatement of antsrl_pop_record_pre / _post member by
                member (memory_agent_ref.sample_indices and ring_rows with the member's seed and env_id_base + p Em).
  collect step  TRAIN, train_case and train_inputs: linear_train_cases.inputs per member (its `member` argument), with the
                member's own discount; the reference is linear_train_ref.contract_train_step under fp32_sum_bounds.
  launch rules  pol_flat_lds, pol_flat_fits, pop_policy_blocks, lt_lds restated from antsrl_policy_flat.h,
                antsrl_population.h and antsrl_lintrain.hip, and what they make of a case (acting_launch)."""
from functools import lru_cache

import numpy as np
import torch

import linear_train_cases as K
import memory_agent_ref as R
from dqn_ref import U_FP32, bf16, gamma  # noqa: F401

POP_MAX = 64  # include/antsrl.h ANTSRL_POP_MAX
LDS_PLAIN = 64 * 1024   # dynamic LDS a kernel gets without the opt-in
LDS_CU = 160 * 1024     # a CU's LDS


# ---- the launch rules, restated ----------------------------------------------------------------------------------------
def pol_flat_tile_elems(F):
    return (32 * F + 32 + 7) // 8 * 8


def pol_flat_lds(F):
    """antsrl_policy_flat.h: W1's observation columns as bf16 [32][16 ksteps + 8] and two tile images."""
    ks = (F + 15) // 16
    return 32 * (16 * ks + 8) * 2 + 2 * pol_flat_tile_elems(F) * 2


def pol_flat_fits(F):
    return (F + 15) // 16 <= 64 and pol_flat_lds(F) <= LDS_CU


def pop_policy_blocks(Mm, F, P):
    """antsrl_population.h -> (workgroups per member, the workgroups wanted, the cap, resident workgroups per CU)."""
    per_cu = min(max(LDS_CU // pol_flat_lds(F), 1), 8)
    ntiles = (Mm + 31) // 32
    want = (ntiles + 1) // 2
    cap = (256 * per_cu + P - 1) // P
    return min(want, cap), want, cap, per_cu


lt_lds = K.lds_bytes  # antsrl_lintrain.hip's, as linear_train_cases restates it (NW = 4: k_pop_lintrain's)


def acting_launch(case):
    """What the launch rule makes of an acting case: lds, blocks, want, cap, per_cu, ntiles and, per wave of a member's
    2 * blocks waves, the rows of the tiles it takes in turn."""
    Mm, F, P = case["Em"] * case["N"], case["F"], case["P"]
    blocks, want, cap, per_cu = pop_policy_blocks(Mm, F, P)
    ntiles, nwaves = (Mm + 31) // 32, 2 * blocks
    waves = [[min(32, Mm - 32 * t) for t in range(w, ntiles, nwaves)] for w in range(nwaves)]
    return dict(lds=pol_flat_lds(F), blocks=blocks, want=want, cap=cap, per_cu=per_cu, ntiles=ntiles, waves=waves)


# ---- acting ------------------------------------------------------------------------------------------------------------
# `seed`: the rows' and nets' generator.  The 8-row and 1-row cases carry seeds at which the shares of clear rows and the
# wrong readings of test_population_stage_cases_cpu.py hold (found on the references alone: the first seed from 0 on).
ACTING = {
    "A1": dict(P=3, Em=2, N=4, F=9, seed=1),      # F < 16, one partial k-step, odd F; one tile of 8 rows
    "A2": dict(P=3, Em=1, N=36, F=50, seed=0),    # F % 16 = 2; a whole tile and one of 4 rows
    "A3": dict(P=2, Em=1, N=104, F=343, seed=0),  # odd F at 7 x 7 x 7; LDS 67 072 B: the opt-in; two workgroups per member
    "A4": dict(P=2, Em=1, N=34, F=848, seed=0),   # the widest row: 163 456 of 163 840 B
    "A4-one": dict(P=1, Em=1, N=1, F=848, seed=0),  # Mm = 1
    "A5": dict(P=64, Em=4, N=137, F=294, seed=0),  # P at its maximum; cap 8 < 9 workgroups: waves loop, tile 17 has 4 rows
}
ACTING_IDS = list(ACTING)
CLEAR_SHARE = 0.8  # of a member's rows, per head


def _linear(g, out_f, in_f):
    b = in_f ** -0.5
    return (torch.rand((out_f, in_f), generator=g) * 2 - 1) * b, (torch.rand((out_f,), generator=g) * 2 - 1) * b


def acting_inputs(case, seed=None):
    """Per member p: w1 [32, F + 2], b1, w2 [3, 32], b2 (layer1 and the LIVE layer2), w3, b3 (the live layer3) and tw3, tb3
    (the target's), all fp32 of nn.Linear's init; obs [P, Mm, F] fp32 holding bfloat16 values in (-1, 1); ast [P, Mm, 2]
    fp32 in [0, 5).  Returned stacked over the members."""
    P, Mm, F = case["P"], case["Em"] * case["N"], case["F"]
    g = torch.Generator().manual_seed(7919 * F + 31 * P + Mm + 104729 * (case["seed"] if seed is None else seed))
    nets = {k: [] for k in ("w1", "b1", "w2", "b2", "w3", "b3", "tw3", "tb3")}
    for _ in range(P):
        for names, (o, i) in ((("w1", "b1"), (32, F + 2)), (("w2", "b2"), (3, 32)), (("w3", "b3"), (3, 32)), (("tw3", "tb3"), (3, 32))):
            w, b = _linear(g, o, i)
            nets[names[0]].append(w)
            nets[names[1]].append(b)
    out = {k: torch.stack(v) for k, v in nets.items()}
    out["obs"] = bf16(torch.rand((P, Mm, F), generator=g) * 2 - 1)
    out["ast"] = torch.rand((P, Mm, 2), generator=g) * 5
    return out


def _spacing(h):
    """bfloat16's spacing at |h| (float64): 2^(e - 7) in the binade 2^e of h; the smallest normal's below it."""
    e = torch.floor(torch.log2(h.abs().clamp_min(2.0 ** -126)))
    return 2.0 ** (e - 7)


def acting_forward(inp, p, net=None, l3="target", rows=None):
    """Member p's rows through member `net`'s net (default p's own) in float64 on the bfloat16-rounded observations,
    agent states and weights, the hidden values rounded to bfloat16 before the heads.  l3: "target" (the acting net's,
    collect_agent.py:166) or "live".  rows: ([Mm, F], [Mm, 2]) in place of the member's own.
    -> (q [Mm, 6]: rotation then pheromone, bound [Mm, 6]).

    The bound, per row and output, on |device - q|, derived and not measured.  The device sums layer1 in fp32 in an order
    of its own: F + 2 products (exact in fp32) and the bias, at most F + 3 roundings, e_h = gamma(F + 3) (|x| |w1|^T + |b1|).
    Its hidden value then rounds to bfloat16 where the exact one may round the other way: one bfloat16 spacing (e_h is
    far below a spacing: a sum cannot skip a value).  Both pass through |w2|; the head's own fp32 sum of 32 exact products
    and a bias adds gamma(34) (|h| |w2|^T + |b2|)."""
    q = p if net is None else net
    x, a = (inp["obs"][p], inp["ast"][p]) if rows is None else rows
    F = x.shape[1]
    w1 = bf16(inp["w1"][q]).double()
    b1 = inp["b1"][q].double()
    xa = torch.cat([bf16(x), bf16(a)], 1).double()
    h = xa @ w1.T + b1
    eh = gamma(F + 3) * (xa.abs() @ w1.abs().T + b1.abs())
    hb = bf16(h.float()).double()
    w3, b3 = (inp["tw3"][q], inp["tb3"][q]) if l3 == "target" else (inp["w3"][q], inp["b3"][q])
    W = bf16(torch.cat([inp["w2"][q], w3])).double()
    b = torch.cat([inp["b2"][q], b3]).double()
    out = hb @ W.T + b
    bound = (_spacing(hb) + eh) @ W.abs().T + gamma(34) * (hb.abs() @ W.abs().T + b.abs())
    return out, bound


def decide(q):
    """Both heads' actions of q [M, 6] -> (rotation - 1 as the kernel writes it, pheromone), int64 [M]: the first
    maximum wins, as the body's comparisons have it (and torch.max's indices)."""
    def first(v):
        a = (v[:, 1] > v[:, 0]).long()
        return torch.where(v[:, 2] > v.gather(1, a[:, None])[:, 0], torch.full_like(a, 2), a)
    return first(q[:, :3]) - 1, first(q[:, 3:])


def clear_rows(q, bound):
    """[M, 2] bool: per head, whether the row's top-2 margin exceeds twice the row's largest bound on that head."""
    out = []
    for s in (slice(0, 3), slice(3, 6)):
        top = q[:, s].topk(2, dim=1).values
        out.append((top[:, 0] - top[:, 1]) > 2 * bound[:, s].max(dim=1).values)
    return torch.stack(out, 1)


@lru_cache(maxsize=None)
def acting_case(name):
    """The case with its inputs and per member its reference: rot, ph [P, Mm] int64 and clear [P, Mm, 2] bool.  Computed
    once and shared: nobody writes into it."""
    case = dict(ACTING[name], name=name)
    inp = acting_inputs(case)
    rot, ph, clear = [], [], []
    for p in range(case["P"]):
        q, bound = acting_forward(inp, p)
        r, f = decide(q)
        rot.append(r)
        ph.append(f)
        clear.append(clear_rows(q, bound))
    return dict(case, Mm=case["Em"] * case["N"], inp=inp, rot=torch.stack(rot), ph=torch.stack(ph), clear=torch.stack(clear))


def explore_blocks(inp):
    """[P, 32 (F + 2) + 131]: ExploreTrainer's flat block per member (layer1.weight, layer1.bias, layer2.weight,
    layer2.bias) of the members' w1, b1, w2, b2."""
    P = inp["w1"].shape[0]
    return torch.cat([inp["w1"].reshape(P, -1), inp["b1"], inp["w2"].reshape(P, -1), inp["b2"]], 1).contiguous()


# ---- select ------------------------------------------------------------------------------------------------------------
def _cycle(values, P):
    return tuple(values[p % len(values)] for p in range(P))


# members 0 and 2 share a seed wherever there are three; epsilons 0, 0.5 and 1 all occur
SELECT = {
    "S1": dict(P=3, Em=2, N=20, base=0, step=4, seeds=(7, 8, 7), eps=(0.0, 0.5, 1.0)),
    "S2-P64": dict(P=64, Em=1, N=1, base=0, step=9, seeds=_cycle((3, 4, 3, 11, 12), 64), eps=_cycle((0.5, 0.0, 1.0, 0.5), 64)),
    "S3-base-step": dict(P=5, Em=7, N=33, base=11, step=(1 << 40) + 3, seeds=(5, 6, 5, 1 << 61, 9), eps=(0.5, 0.5, 1.0, 0.0, 0.5)),
    "S4-blocks": dict(P=2, Em=300, N=3, base=0, step=2, seeds=(21, 22), eps=(0.5, 0.5)),  # 900 ants: four workgroups a member
}
SELECT_IDS = list(SELECT)


def select_inputs(case):
    """What the buffers hold before the call: rot in {-1, 0, 1} and ph in {0, 1, 2}, int8 [P Em, N]."""
    rng = np.random.default_rng(case["P"] * 1000 + case["N"])
    E = case["P"] * case["Em"]
    return rng.integers(-1, 2, (E, case["N"])).astype(np.int8), rng.integers(0, 3, (E, case["N"])).astype(np.int8)


def select_expected(case, rot, ph):
    """memory_agent_ref.select member by member with the member's seed and epsilon and env_id_base + p Em."""
    Em, N = case["Em"], case["N"]
    out_r, out_p, out_e = rot.copy(), ph.copy(), np.zeros((case["P"] * Em,), dtype=bool)
    none = np.zeros((Em, N, 0), np.float32)
    for p in range(case["P"]):
        e = slice(p * Em, (p + 1) * Em)
        out_r[e], out_p[e], _, out_e[e] = R.select(case["seeds"][p], case["step"], case["base"] + p * Em, case["eps"][p], 3, 3,
                                                   rot[e], ph[e], none, none)
    return out_r, out_p, out_e


# ---- record ------------------------------------------------------------------------------------------------------------
# R1: F = 343 is odd and max_len 75 too, so the members' slabs of `states` start 75 * 343 * 4 = 102 900 bytes apart, at
# 16-byte phases 0, 4, 8 (the copy's `h`), and a member's bfloat16 rows 66 * 343 * 2 = 45 276 bytes apart with rows of
# 686 bytes: sources at every alignment the copy tells apart (`mode` 0 / 1 / 2).  Rows 65 .. 74 then 0 .. 13: the launch wraps.
# R2: K = 66 > max_len = 50: j0 = 16, only the last 50 entries land (50 is no multiple of the four entries a workgroup takes).
RECORD = {
    "R1": dict(P=3, Em=2, N=33, space=(7, 7, 7), max_len=75, K=24, base=5, head=65, step=6, seeds=(7, 8, 7), pheromone=True),
    "R2": dict(P=3, Em=2, N=33, space=(7, 7, 7), max_len=50, K=None, base=5, head=45, step=6, seeds=(7, 8, 7), pheromone=True),
    "R3": dict(P=64, Em=1, N=5, space=(3, 3, 1), max_len=7, K=3, base=0, head=5, step=2, seeds=_cycle((3, 4, 3, 11, 12), 64),
               pheromone=False),  # the explore population's ring: no pheromone, the ring stores 1
}
RECORD_IDS = list(RECORD)
FILL_ACTION, FILL_DONE = -77, 7  # what ring rows hold that nothing wrote (the float arrays: NaN)


def record_inputs(case):
    """One step's buffers as numpy: obs0 / obs1 [P Mm, F] fp32 on bfloat16 values (before and after the environment's
    step), ast0 / ast1 [P Mm, 2], rot, ph int8 [P Mm], reward [P Mm] and done uint8 [P Em], which differs per environment."""
    P, Em, N, F = case["P"], case["Em"], case["N"], int(np.prod(case["space"]))
    M = P * Em * N
    g = torch.Generator().manual_seed(F + 13 * P + case["max_len"])
    r = lambda *s: torch.rand(s, generator=g)  # noqa: E731
    done = (torch.arange(P * Em) * 7 // 3) % 2  # 0 1 0 1 1 0 ...: no period of Em or of one
    return dict(obs0=bf16(r(M, F) * 2 - 1).numpy(), obs1=bf16(r(M, F) * 2 - 1).numpy(), ast0=r(M, 2).numpy(), ast1=r(M, 2).numpy(),
                rot=torch.randint(-1, 2, (M,), generator=g).to(torch.int8).numpy(),
                ph=torch.randint(0, 3, (M,), generator=g).to(torch.int8).numpy(),
                reward=(r(M) * 4 - 2).numpy(), done=done.to(torch.uint8).numpy())


def record_expected(case, inp):
    """The seven arrays [P, max_len, ...] after record_pre and record_post of one step into rings filled with NaN,
    FILL_ACTION and FILL_DONE, and the rows [P, max_len] bool that were written."""
    P, Em, N, L, F = case["P"], case["Em"], case["N"], case["max_len"], int(np.prod(case["space"]))
    Mm = Em * N
    k = Mm if case["K"] is None else case["K"]
    nan = lambda *s: np.full(s, np.nan, np.float32)  # noqa: E731
    out = dict(states=nan(P, L, F), agent_states=nan(P, L, 2), actions=np.full((P, L, 2), FILL_ACTION, np.int64), rewards=nan(P, L),
               new_states=nan(P, L, F), new_agent_states=nan(P, L, 2), dones=np.full((P, L), FILL_DONE, np.uint8))
    written = np.zeros((P, L), dtype=bool)
    for p in range(P):
        ants = R.sample_indices(case["seeds"][p], case["step"], case["base"] + p * Em, Mm, k)
        js, rows, _ = R.ring_rows(case["head"], L, k)
        a = ants[js]
        g = p * Mm + a  # the ants among the whole batch's
        out["states"][p, rows], out["new_states"][p, rows] = inp["obs0"][g], inp["obs1"][g]
        out["agent_states"][p, rows], out["new_agent_states"][p, rows] = inp["ast0"][g], inp["ast1"][g]
        out["actions"][p, rows, 0] = inp["rot"][g].astype(np.int64) + 1
        out["actions"][p, rows, 1] = inp["ph"][g] if case["pheromone"] else 1
        out["rewards"][p, rows] = inp["reward"][g]
        out["dones"][p, rows] = inp["done"][p * Em + a // N]
        written[p, rows] = True
    return out, written


# ---- the collect step ----------------------------------------------------------------------------------------------------
# the first three are P = 3's; P = 64 goes through all five in turn, so that members 63 and 0 differ as every other pair of
# neighbours does
TRAIN_SEEDS, TRAIN_DISCOUNT, TRAIN_LR = (7, 8, 7, 9, 10), (0.5, 0.99, 0.9, 0.7, 0.3), (1e-3, 1e-4, 3e-3, 3e-4, 1e-2)
TRAIN = {"F%d-B%d" % (F, B): dict(P=3, F=F, B=B, N=600) for F in (9, 50, 294, 1022) for B in (1, 33, 264, 512)}
TRAIN["P64-F50-B33"] = dict(P=64, F=50, B=33, N=100)
TRAIN_IDS = list(TRAIN)


def train_case(name):
    """The case with, per member, its seed, discount and learning rate and the linear_train_cases case its inputs are
    drawn from."""
    c = dict(TRAIN[name], name=name)
    P = c["P"]
    c["seeds"], c["discount"], c["lr"] = _cycle(TRAIN_SEEDS, P), _cycle(TRAIN_DISCOUNT, P), _cycle(TRAIN_LR, P)
    c["members"] = [K._case("%s-m%d" % (name, p), c["F"], c["B"], c["N"], discount=c["discount"][p], **K._wide(c["F"]))
                    for p in range(P)]
    return c


def train_inputs(c, p):
    """linear_train_cases.inputs of member p (its own seed: every tensor differs between members) with a second index
    tensor for the second step, the first one's rows in another order; `ring`: the arrays with NaN in every row that no
    index selects."""
    inp = K.inputs(c["members"][p], member=p)
    g = torch.Generator().manual_seed(K.input_seed(c["members"][p], p) + 1)
    inp["idx2"] = inp["idx"][torch.randperm(c["B"], generator=g)]
    unused = torch.ones((c["N"],), dtype=torch.bool)
    unused[inp["idx"]] = False
    ring = [a.clone() for a in inp["arrays"]]
    for i in (0, 1, 3, 4, 5):
        ring[i][unused] = float("nan")
    inp["ring"] = tuple(ring)
    return inp
