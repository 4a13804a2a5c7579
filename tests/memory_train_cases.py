"""The shapes and inputs at which the memory agent's training step is tested stage by stage and bit for bit:
one list each, shared by the device tests (test_gpu_memory_train_stages.py) and by the CPU test that shows the exact
cases exact and the stage bound sharp (test_memory_train_bounds_cpu.py).  Everything here is CPU torch from seeded
generators.

EXACT cases: inputs for which every fp32 sum of the step is exact, so that the result does not depend on summation order
or on where the launches are cut, and a device must equal float64 bit for bit.  Weights in {0, +-1} (in >= out: the
columns dealt out among the rows, W[c % out][perm[c]]; out > in: one nonzero per row, W[r][perm[r % in]]; no column is
all zero), biases, observations and agent states in {-1, 0, 1} (a share `density` of them nonzero; the last unit of
each ReLU layer has bias +1, so that it is not dead for every row), rewards small integers, discount 0.5, n_rot = n_ph = 32
and B a power of two, so that 2 / (B n) is a power of two.  `exact_trace` is the step in float64 with NO rounding at
all; test_memory_train_bounds_cpu.py asserts that every rounding the contract makes would have been the identity.

STAGE cases: ordinary real-valued data (observations 30 % nonzero in (0, 1), agent states in (-1, 1), normal rewards,
nn.Linear's default init, a target net of its own), at the smallest shapes at which each guard of the kernels is
crossed."""
import torch

from memory_train_ref import IN_OF, TRAINED, layer_dims
from memory_policy_ref import LAYERS


def _case(name, F, power, mem, B, n_rot=3, n_ph=3, idx="none", dones="mixed", discount=0.5, oor=False, nan=False, density=0.3, salt=0):
    return dict(name=name, F=F, power=power, mem=mem, B=B, n_rot=n_rot, n_ph=n_ph, idx=idx, dones=dones,
                discount=discount, oor=oor, nan=nan, density=density, salt=salt)


def dims(c):
    return c["F"], c["power"], c["mem"], c["n_rot"], c["n_ph"]


# ---- the exact cases (salt and density: the first seed and input density at which the premise of
# test_memory_train_bounds_cpu.py holds, coverage included): D % 32 in {0, 1, 16, 28, 31}, D = 4 and 1024, mem in {1, 3, 20, 32}, both powers, every B
_E = dict(n_rot=32, n_ph=32)
EXACT = [
    _case("F1-p4-m1-B32", 1, 4, 1, 32, salt=28, **_E),                 # D = 4
    _case("F27-p4-m3-B64", 27, 4, 3, 64, salt=1, **_E),                 # D = 32
    _case("F61-p4-m1-B2048", 61, 4, 1, 2048, salt=2, **_E),              # D = 64, nchunk 8
    _case("F294-p5-m20-B256", 294, 5, 20, 256, salt=3, **_E),            # D = 316 = 28 mod 32
    _case("F990-p5-m32-B512", 990, 5, 32, 512, **_E),              # D = 1024, nchunk 2
    _case("F11-p4-m20-B1", 11, 4, 20, 1, **_E),                    # D = 33 = 1 mod 32, one row
    _case("F45-p5-m1-B16", 45, 5, 1, 16, density=0.2, salt=6, **_E),                # D = 48 = 16 mod 32, half a row tile
    _case("F28-p4-m1-B32768", 28, 4, 1, 32768, salt=5, **_E),            # D = 31, nchunk 64
    _case("F27-p4-m3-B64-idx", 27, 4, 3, 64, idx="ring", nan=True, salt=1, **_E),
    _case("F27-p4-m3-B64-dones-all", 27, 4, 3, 64, dones="all", salt=1, **_E),
    _case("F27-p4-m3-B64-dones-none", 27, 4, 3, 64, dones="none", salt=1, **_E),
    _case("F27-p4-m3-B64-actions", 27, 4, 3, 64, oor=True, salt=1, **_E),
]
EXACT_IDS = [c["name"] for c in EXACT]

# ---- the stage cases (power 4 unless named)
STAGE = []
for _F in (1, 11, 27, 28, 29, 59, 294, 990, 1019):                 # mem 3: D = 6 16 32 33 34 64 299 995 1024
    STAGE.append(_case("F%d-B33" % _F, _F, 4, 3, 33))
for _m in (1, 20, 32):                                             # D = 31 50 62
    STAGE.append(_case("F28-m%d-B33" % _m, 28, 4, _m, 33))
for _r, _p in ((1, 1), (32, 32), (1, 32)):
    STAGE.append(_case("F27-heads%dx%d-B33" % (_r, _p), 27, 4, 3, 33, n_rot=_r, n_ph=_p))
for _B in (1, 31, 32, 256, 257, 264, 289, 513, 16385):             # 33 is above
    STAGE.append(_case("F27-B%d" % _B, 27, 4, 3, _B))
STAGE.append(_case("F294-p5-m20-B264", 294, 5, 20, 264))
STAGE += [
    _case("F27-B40-noidx", 27, 4, 3, 40),
    _case("F27-B40-idx", 27, 4, 3, 40, idx="ring"),
    _case("F27-B40-idx-nan", 27, 4, 3, 40, idx="ring", nan=True),
    _case("F27-B40-discount-0", 27, 4, 3, 40, discount=0.0),
    _case("F27-B40-discount-0.99", 27, 4, 3, 40, discount=0.99),
    _case("F27-B40-dones-all", 27, 4, 3, 40, dones="all"),
    _case("F27-B40-dones-none", 27, 4, 3, 40, dones="none"),
    _case("F27-B40-actions", 27, 4, 3, 40, oor=True),
]
STAGE_IDS = [c["name"] for c in STAGE]


def _seed(c):
    return 7919 * c["F"] + 131 * c["B"] + 17 * c["mem"] + c["power"] + 3 * c["n_rot"] + 5 * c["n_ph"] + 1000003 * c["salt"]


def _finish(c, g, arrays):
    """dones mode, out-of-range actions, and the ring: (arrays over N rows, idx or None).  With idx, the B rows are
    scattered into a ring of N = B + B // 2 + 3 rows through a permutation with repeats (row 0 of the minibatch is taken
    three times); with nan, every row of the ring that idx does not select is NaN in all five float arrays."""
    st, ast, act, rw, nst, nast, dn = arrays
    B = c["B"]
    if c["dones"] != "mixed":
        dn[:] = c["dones"] == "all"
    elif B >= 2:
        dn[0], dn[1] = True, False
    if c["oor"]:
        act = act.clone()
        act[0:B - 1:7, 0] = -1      # not the last row: it holds the last action of both heads
        act[1:B - 1:5, 1] = c["n_ph"]
        act[2:B - 1:11, 0] = 99
        act[3:B - 1:13, 1] = -(1 << 40)
    arrays = (st, ast, act, rw, nst, nast, dn)
    if c["idx"] == "none":
        return arrays, None
    N = B + B // 2 + 3
    where = torch.randperm(N, generator=g)[:B]
    if B >= 4:  # repeats: rows 1 and 2 of the minibatch are row 0 again
        for t in arrays:
            t[1], t[2] = t[0].clone(), t[0].clone()
        where[1], where[2] = where[0], where[0]
    ring = []
    for t in arrays:
        fill = float("nan") if (c["nan"] and t.dtype == torch.float32) else 0
        r = torch.full((N,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
        r[where] = t
        ring.append(r)
    return tuple(ring), where.clone()


def gathered(arrays, idx):
    return arrays if idx is None else tuple(t[idx] for t in arrays)


def _memory_head(g, c, sd):
    shapes = layer_dims(*dims(c))
    for name, (o, i) in zip(LAYERS[9:], shapes[9:]):
        sd[name + ".weight"] = (torch.rand((o, i), generator=g) * 2 - 1) * i ** -0.5
        sd[name + ".bias"] = (torch.rand((o,), generator=g) * 2 - 1) * i ** -0.5
    return sd


# ======================================================================================================================
# exact cases
# ======================================================================================================================
def _exact_net(g, c):
    sd = {}
    for name, (o, i) in zip(TRAINED, layer_dims(*dims(c))[:9]):
        W = torch.zeros((o, i))
        sg = (torch.randint(0, 2, (o, i), generator=g) * 2 - 1).float()
        perm = torch.randperm(i, generator=g)
        if i >= o:
            cc = torch.arange(i)
            W[cc % o, perm[cc]] = sg[cc % o, perm[cc]]
        else:
            rr = torch.arange(o)
            W[rr, perm[rr % i]] = sg[rr, perm[rr % i]]
        sd[name + ".weight"] = W
        b = (torch.randint(0, 2, (o,), generator=g) * 2 - 1).float() * (torch.rand((o,), generator=g) < c["density"])
        if name in TRAINED[:3]:
            b[o - 1] = 1.0  # the last ReLU unit is not dead for every row: dW's last row and the next layer's last column
        sd[name + ".bias"] = b
    return _memory_head(g, c, sd)


def exact_inputs(c):
    """-> dict(sd, target, arrays, idx): the model's and the target's 26 tensors, the replay arrays, idx or None."""
    g = torch.Generator().manual_seed(_seed(c))
    F, mem, B = c["F"], c["mem"], c["B"]
    sd, target = _exact_net(g, c), _exact_net(g, c)

    def tern(*shape):
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * (torch.rand(shape, generator=g) < c["density"])
    st, nst = tern(B, F), tern(B, F)
    ast, nast = tern(B, 2 + mem), tern(B, 2 + mem)
    act = torch.stack([torch.randint(0, c["n_rot"], (B,), generator=g), torch.randint(0, c["n_ph"], (B,), generator=g)], 1)
    act[B - 1, 0], act[B - 1, 1] = c["n_rot"] - 1, c["n_ph"] - 1  # the last row of both heads' dW gets a term
    rw = torch.randint(-2, 3, (B,), generator=g).float()
    dn = torch.rand((B,), generator=g) < 0.2
    arrays, idx = _finish(c, g, (st, ast, act, rw, nst, nast, dn))
    return dict(sd=sd, target=target, arrays=arrays, idx=idx)


def exact_trace(c, inp):
    """The step in float64 with no rounding anywhere (the arithmetic of memory_train_ref.bf16_train_grads without its
    bf16 roundings): loss, grads by name, and every tensor that the contract rounds or sums, for the premise test."""
    st, ast, act, rw, nst, nast, dn = gathered(inp["arrays"], inp["idx"])
    B = st.shape[0]
    M = {k: v.double() for k, v in inp["sd"].items()}
    T = {k: v.double() for k, v in inp["target"].items()}
    x, xn = torch.cat([st, ast], 1).double(), torch.cat([nst, nast], 1).double()
    rounded, sums = [], []   # (what, tensor) at a bf16 rounding point; (what, |a| |w| sum, lowest bit of a term)

    def lin(P, n, t, tag):
        rounded.append((tag + " input of " + n, t))
        extra = (xn if tag == "target" else x).abs() if n == "layer4" else 0.0   # the residual joins the same fp32 value
        low = min(_lsb(t) * _lsb(P[n + ".weight"]), _lsb(P[n + ".bias"]), 1.0)      # x and the biases are integers
        sums.append((tag + " " + n, t.abs() @ P[n + ".weight"].abs().T + P[n + ".bias"].abs() + extra, low))
        return t @ P[n + ".weight"].T + P[n + ".bias"]

    def fwd(P, x, tag):
        o = {}
        o["layer1"] = torch.relu(lin(P, "layer1", x, tag))
        o["layer2"] = torch.relu(lin(P, "layer2", o["layer1"], tag))
        o["layer3"] = torch.relu(lin(P, "layer3", o["layer2"], tag))
        o["layer4"] = lin(P, "layer4", o["layer3"], tag) + x
        for n in TRAINED[4:]:
            o[n] = lin(P, n, o[TRAINED[IN_OF[TRAINED.index(n)]]], tag)
        return o
    to, mo = fwd(T, xn, "target"), fwd(M, x, "model")
    nd = torch.where(dn, 0.0, 1.0).double()
    loss, dout, terms = 0.0, {}, []
    for head, col in (("rotation_layer3", 0), ("pheromone_layer2", 1)):
        q, n = mo[head], mo[head].shape[1]
        a = act[:, col]
        ok = (a >= 0) & (a < n)
        y = rw.double() + 0.5 * to[head].max(1).values * nd
        d = torch.where(ok, q.gather(1, a.clamp(0, n - 1).view(-1, 1)).view(-1) - y, torch.zeros_like(y))
        dq = torch.zeros_like(q)
        r = ok.nonzero().view(-1)
        dq[r, a[r]] = d[r] * (2.0 / (B * n))
        dout[head] = dq
        terms.append(d * d * (1.0 / (B * n)))
        loss = loss + terms[-1].sum()
    sums.append(("loss", (terms[0] + terms[1]).sum().view(1), min(_lsb(terms[0]), _lsb(terms[1]))))

    def back(n):
        rounded.append(("dOut of " + n, dout[n]))
        sums.append(("backward of " + n, dout[n].abs() @ M[n + ".weight"].abs(), _lsb(dout[n]) * _lsb(M[n + ".weight"])))
        return dout[n] @ M[n + ".weight"]
    dout["rotation_layer2"] = back("rotation_layer3")
    dout["pheromone_layer1"] = back("pheromone_layer2")
    dout["rotation_layer1"] = back("rotation_layer2")
    b1, b2 = back("rotation_layer1"), back("pheromone_layer1")
    sums.append(("dg, both segments", sums[-1][1] + sums[-2][1], min(sums[-1][2], sums[-2][2])))
    dout["layer4"] = b1 + b2
    dout["layer3"] = back("layer4") * (mo["layer3"] > 0)
    dout["layer2"] = back("layer3") * (mo["layer2"] > 0)
    dout["layer1"] = back("layer2") * (mo["layer1"] > 0)
    rounded.append(("dOut of layer1", dout["layer1"]))
    grads = {}
    for l, n in enumerate(TRAINED):
        inp_ = x if IN_OF[l] < 0 else mo[TRAINED[IN_OF[l]]]
        rounded.append(("saved input of " + n, inp_))
        grads[n + ".weight"] = dout[n].T @ inp_
        grads[n + ".bias"] = dout[n].sum(0)
        sums.append(("dW of " + n, dout[n].abs().T @ inp_.abs(), _lsb(dout[n]) * _lsb(inp_)))
        sums.append(("db of " + n, dout[n].abs().sum(0), _lsb(dout[n])))
    return dict(loss=loss, grads=grads, rounded=rounded, sums=sums)


def _lsb(t):
    """The lowest set bit over the nonzero elements of t (float64), as a power of two; 1.0 for an all-zero tensor."""
    v = t[t != 0].abs().double()
    if v.numel() == 0:
        return 1.0
    m, e = torch.frexp(v)                       # v = m 2^e, m in [0.5, 1): m 2^53 is an integer
    k = (m * 2.0 ** 53).to(torch.int64)
    low = (k & -k).double()                     # its lowest set bit
    return float((low * 2.0 ** (e.double() - 53)).min())


def flat(grads):
    return torch.cat([grads[n + s].reshape(-1) for n in TRAINED for s in (".weight", ".bias")])


# ======================================================================================================================
# stage cases
# ======================================================================================================================
def _linear_net(g, c):
    sd = {}
    for name, (o, i) in zip(TRAINED, layer_dims(*dims(c))[:9]):
        sd[name + ".weight"] = (torch.rand((o, i), generator=g) * 2 - 1) * i ** -0.5
        sd[name + ".bias"] = (torch.rand((o,), generator=g) * 2 - 1) * i ** -0.5
    return _memory_head(g, c, sd)


def stage_inputs(c):
    """-> dict(sd, target, arrays, idx, stale): `stale` holds, per net, the nine weights of "the step before": one Adam
    step of lr 1e-4 back (every element moved by 1e-4 one way or the other), what a pack that apply() left stale or
    sync_target() did not carry would still hold."""
    g = torch.Generator().manual_seed(_seed(c))
    F, mem, B = c["F"], c["mem"], c["B"]
    sd, target = _linear_net(g, c), _linear_net(g, c)

    def obs():
        return (torch.rand((B, F), generator=g) < 0.3).float() * torch.rand((B, F), generator=g)

    def agent():
        return torch.rand((B, 2 + mem), generator=g) * 2 - 1
    st, ast = obs(), agent()
    act = torch.stack([torch.randint(0, c["n_rot"], (B,), generator=g), torch.randint(0, c["n_ph"], (B,), generator=g)], 1)
    rw = torch.randn((B,), generator=g)
    nst, nast = obs(), agent()
    dn = torch.rand((B,), generator=g) < 0.3
    arrays, idx = _finish(c, g, (st, ast, act, rw, nst, nast, dn))
    stale = [[d[n + ".weight"] + 1e-4 * (torch.randint(0, 2, d[n + ".weight"].shape, generator=g) * 2 - 1).float() for n in TRAINED]
             for d in (target, sd)]
    return dict(sd=sd, target=target, arrays=arrays, idx=idx, stale=stale)
