"""The shapes and inputs at which the linear agent's training step is tested beyond F = 294 ("The step at
other shapes"): one list, shared by the device tests (test_gpu_linear_train_shapes.py) and by the CPU test that shows
linear_train_ref.fp32_sum_bounds safe and sharp at the same shapes (test_linear_train_bounds_cpu.py).

Everything here is CPU torch from a seeded generator.  inputs(case) gives
    sd        the six tensors under CollectModel's names (nn.Linear's default init)
    target    (w3, b3) of the target net: not the model's
    arrays    the replay arrays (states [N, F], agent_states [N, 2], actions [N, 2] int64, rewards [N], new_states,
              new_agent_states, dones [N] bool)
    idx       int64 [B], or None (rows 0 .. B - 1)
    raw       idx / actions before the contract's clamps, where the case has some (else None)
Observations: half of them zero, the others signed, a share `big` of them log-uniform in [2^-10, 2^10] and the rest
uniform in (-1, 1); one in eight of the non-zero ones is an exact bfloat16 tie +-(1 + 2^-8) 2^e or +-(1 + 3 2^-8) 2^e (round
to nearest even takes the first down and the second up; truncation and round-half-up each get one of them wrong).  Every
row holds at least one tie of each kind where F >= 3.  Column F - 1 is dense and large (2^8 .. 2^10), so that a kernel
which drops it moves every row by more than gamma(F + 3) of the row's sum at every width.
Agent states are signed, |a| log-uniform in [1, 2^as_exp], and every one of them lies a fifth of a bfloat16 spacing above a
bfloat16 value: left unrounded, they move every row's q the same way instead of cancelling over the batch.
Rewards make the rotation head's TD error small (|d| about 2^-12 |q|), as a trained net's is: the bound's row-sum term
gamma(B + 2) sum |d| |h| then stays below what a wrong rounding does even at B = 131 233, where gamma(B + 2) = 0.8 %
exceeds bfloat16's whole unit roundoff.  The pheromone head's TD error is whatever the shared reward leaves: O(|q|).
The ring row in the batch's last place is the exception: its TD error is 4 (|q| + 1), so that a sum which leaves the last
row out is off by more than the other rows' bounds together."""
import torch

NAMES = ("explore_model.layer1.weight", "explore_model.layer1.bias", "explore_model.layer2.weight",
         "explore_model.layer2.bias", "layer3.weight", "layer3.bias")


def _case(name, F, B, N, idx="rand", discount=0.5, dones="mixed", clamp=None, big=1.0, as_exp=10):
    return dict(name=name, F=F, B=B, N=N, idx=idx, discount=discount, dones=dones, clamp=clamp, big=big, as_exp=as_exp)


def _wide(F):
    # Wide rows: gamma(F + 3) grows with F while the defects of the sharpness test do not.  Where layer1 is a sum of
    # ~F / 2 observations of magnitude up to 2^10, an agent state left unrounded (2 of its terms, relative 2^-9) drowns
    # in the bound; so from F = 294 on most observations are O(1) and the agent states are larger.
    return dict(big=0.02, as_exp=14) if F >= 294 else {}


WIDTHS = (1, 7, 9, 15, 16, 17, 32, 343, 607, 608, 609, 1022)  # 608 / 609: either side of 64 KiB of LDS (lds_bytes)
CASES = []
for _F in WIDTHS:
    for _B in (33, 264):
        CASES.append(_case("width-F%d-B%d" % (_F, _B), _F, _B, 300, **_wide(_F)))
for _F in (17, 294):
    for _B in (32, 33, 511, 512, 513, 544):
        CASES.append(_case("seam-F%d-B%d" % (_F, _B), _F, _B, 600, **_wide(_F)))
CASES.append(_case("gridcap-F17-B131233", 17, 131072 + 161, 3000))
for _N in (1, 33, 513):
    CASES.append(_case("noidx-N%d" % _N, 17, _N, _N, idx="none"))
for _N in (1, 2):
    CASES.append(_case("ring-N%d-B40" % _N, 9, 40, _N))
CASES.append(_case("clamp-idx", 17, 40, 50, clamp="idx"))
CASES.append(_case("clamp-actions", 17, 40, 50, clamp="actions"))
CASES.append(_case("discount-0", 17, 264, 300, discount=0.0))
CASES.append(_case("discount-0.99", 17, 264, 300, discount=0.99))
CASES.append(_case("dones-all", 17, 264, 300, dones="all"))
CASES.append(_case("dones-none", 17, 264, 300, dones="none"))
IDS = [c["name"] for c in CASES]

# The shapes at which the workspace is read back (test_gpu_dqn_train_workspace.py), the smallest at which each grid regime
# of the gradient stage exists: 5 workgroups, the last with one tile on wave 0 and three idle waves; 17 tiles; 512
# workgroups of one tile per wave, narrow and at F = 294 without and with dones; 1024 workgroups whose waves loop.
WORKSPACE = [c for c in CASES if c["name"] in ("seam-F17-B513", "seam-F17-B544")]
WORKSPACE.append(_case("full-F17-B65536", 17, 65536, 3000))
WORKSPACE.append(_case("full-F294-B65536-dones-none", 294, 65536, 3000, dones="none", **_wide(294)))
WORKSPACE.append(_case("full-F294-B65536", 294, 65536, 3000, **_wide(294)))
WORKSPACE += [c for c in CASES if c["name"] == "gridcap-F17-B131233"]
WORKSPACE_IDS = [c["name"] for c in WORKSPACE]


def lds_bytes(F, nw=4):
    """Dynamic LDS of the gradient stage at width F (lt_lds, antsrl_lintrain.hip): W1 as bf16 [32][16 ksteps + 8], three
    head slots (304 floats), b1 and two W1 columns (96), and per wave its partials (200) and its h / dq tiles (32 x 33 + 32 x 8)."""
    ksteps = (F + 15) // 16
    return 32 * (16 * ksteps + 8) * 2 + (304 + 96 + nw * 200 + nw * (32 * 33 + 32 * 8)) * 4


def _observations(g, N, F, big):
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    sign = lambda *s: torch.randint(0, 2, s, generator=g).double() * 2 - 1  # noqa: E731
    mag = torch.where(rnd(N, F) < big, 2.0 ** (rnd(N, F) * 20 - 10), rnd(N, F))
    tie = (1 + (1 + 2 * torch.randint(0, 2, (N, F), generator=g).double()) * 2.0 ** -8) * 2.0 ** torch.randint(-3, 4, (N, F), generator=g).double()
    x = torch.where(rnd(N, F) < 0.125, tie, mag) * sign(N, F)
    keep = rnd(N, F) < 0.5
    x = x * keep
    x[:, F - 1] = 2.0 ** (8 + 2 * rnd(N)) * sign(N)  # the last column is dense and large
    if F >= 3:  # a tie of each kind in every row, at columns that move with the row
        r = torch.arange(N)
        x[r, r % (F - 1)] = (1 + 2.0 ** -8) * sign(N)
        x[r, (r + 1) % (F - 1)] = (1 + 3 * 2.0 ** -8) * sign(N)
    return x.float()


def input_seed(case, member=0):
    """The seed of inputs(case, member=member): the case's own for member 0, as it always was."""
    return 1000 * case["F"] + case["B"] + 7 * case["N"] + 1000003 * member


def inputs(case, dones=None, discount=None, member=0):
    """`dones` overrides the case's mode ("mixed", "all", "none") and `discount` its discount.  `member` (a population's:
    population_stage_cases.py) is folded into the seed, so that every member's net, ring and indices differ in every
    tensor; member 0 is the case as it stands."""
    F, B, N = case["F"], case["B"], case["N"]
    discount = case["discount"] if discount is None else discount
    g = torch.Generator().manual_seed(input_seed(case, member))

    def linear(out_f, in_f):
        b = in_f ** -0.5
        return ((torch.rand((out_f, in_f), generator=g) * 2 - 1) * b), ((torch.rand((out_f,), generator=g) * 2 - 1) * b)
    w1, b1 = linear(32, F + 2)
    w2, b2 = linear(3, 32)
    w3, b3 = linear(3, 32)
    tw3, tb3 = linear(3, 32)
    sd = dict(zip(NAMES, (w1, b1, w2, b2, w3, b3)))
    st, nst = _observations(g, N, F, case["big"]), _observations(g, N, F, case["big"])

    def agent_states():
        a = 2.0 ** (torch.rand((N, 2), generator=g, dtype=torch.float64) * case["as_exp"])
        a = (a * (torch.randint(0, 2, (N, 2), generator=g).double() * 2 - 1)).float().to(torch.bfloat16).double()
        spacing = 2.0 ** (torch.floor(torch.log2(a.abs())) - 7)
        return (a + 0.2 * spacing).float()  # exact in fp32; rounds back to a (below a power of two the spacing halves: 0.4 of it)
    ast, nast = agent_states(), agent_states()
    act = torch.randint(0, 3, (N, 2), generator=g)
    mode = dones or case["dones"]
    dn = torch.rand((N,), generator=g) < 0.3
    if mode == "mixed" and N >= 2:
        dn[0], dn[1] = True, False
    elif mode != "mixed" or N == 1:
        dn[:] = mode == "all"
    idx = None if case["idx"] == "none" else torch.randint(0, N, (B,), generator=g)
    if idx is not None and N >= 2:
        idx[0], idx[B - 1] = 0, 1  # both kinds of row are in the batch, one of them in its last place
    raw = None
    if case["clamp"] == "idx":
        raw = idx.clone()
        raw[3], raw[11], raw[32], raw[39] = -5, N, N + 7, 1 << 40
        idx = raw.clamp(0, N - 1)
    elif case["clamp"] == "actions":
        raw = act.clone()
        raw[idx[2], 0], raw[idx[5], 1], raw[idx[33], 0], raw[idx[33], 1] = -1, 3, 7, -1
        act = raw.clamp(0, 2)
    # rewards: the rotation head's TD target lands on its q, up to noise (float64 on the bfloat16-rounded operands)
    r16 = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    hid = lambda x, a: r16(torch.cat([x, a], 1)) @ r16(w1).T + b1.double()  # noqa: E731
    q = (hid(st, ast) @ w2.double().T + b2.double())[torch.arange(N), act[:, 0]]
    qn = (hid(nst, nast) @ w2.double().T + b2.double()).max(dim=1).values
    noise = torch.randn((N,), generator=g, dtype=torch.float64) * 2.0 ** -12 * (q.abs() + 1)
    last = B - 1 if idx is None else int(idx[B - 1])
    noise[last] = 4 * (q[last].abs() + 1)
    rw = (q - discount * qn * (~dn).double() + noise).float()
    return dict(sd=sd, target=(tw3, tb3), arrays=(st, ast, act, rw, nst, nast, dn), idx=idx, raw=raw)


def gathered(inp, B):
    """The minibatch as contract_train_step takes it."""
    idx = inp["idx"] if inp["idx"] is not None else torch.arange(B)
    return tuple(a[idx].numpy() for a in inp["arrays"])
