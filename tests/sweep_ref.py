"""The pheromone sweeps' reference, plan and cases (csrc/antsrl_sweep.hip): what test_sweep_ref_cpu.py proves on the host
and test_gpu_sweep_dense.py holds the kernels to.

  sweep64           one update of Walls then Pheromone without a deposit, float64, from the definition
  sweep_plan        launch_sweep_c's decisions restated: kernel, segment rows, strip width, their counts
  sweep_decomposed  sweep64 computed the way the plan cuts it, (strip, segment) pair by pair, with one defect or none
  fields / walls    dense, near_cut, blocks, impulses; walls forced on / off at the seams
  CASES             the smallest shapes at which every seam of every kernel exists

ROUNDINGS PER OUTPUT (the a-priori bound n * 2^-24 * |ref| of a sum of non-negative terms, `apriori_rtol`).  The kernels
keep every tap as hi + lo (KP::ftap) and accumulate by fmaf: one fp32 rounding per fmaf, the product inside it is exact.
  general march, k_sweep_r1x2   S*S taps x {hi, lo} = 2 S^2 fmaf into the output's accumulator       n = 2 S^2
  separable (march SEP, sep2)   across the lanes: S taps x {hi, lo} = 2S fmaf into h (the first one adds to 0 and still
                                rounds); along the march: S rows x {hi, lo} = 2S fmaf into the accumulator; an error of
                                h reaches the output once, scaled by u[a] >= 0                        n = 4 S
  radius 0                      the product is formed in float64 and rounded to fp32 once              n = 1
Inputs are fp32 already and the float64 reference's own error (<= S^2 * 2^-53) is out of sight.  First order in 2^-24
would do; the bound below is the rigorous gamma_n = n u / (1 - n u).
"""
import numpy as np

from antsrl_amd import config as cm

SW0_UNROLL = 4          # antsrl_sweep.hip:14
SEP2_HL = 4             # antsrl_sweep.hip:438
SCALAR_BLOCK_CAP = 256 * 64  # antsrl_sweep.hip:583
IMPULSE = 200.0


def stencil_filter(radius, separable, seed):
    """Asymmetric filters (no tap equals its mirror image or its transpose), general or rank-1, summing to 0.97."""
    rng = np.random.default_rng(seed)
    if separable:
        f = np.outer(0.2 + rng.random(2 * radius + 1), 0.2 + rng.random(2 * radius + 1))  # asymmetric rank-1
    else:
        f = 0.1 + rng.random((2 * radius + 1, 2 * radius + 1))
    return f / f.sum() * 0.97


# ------------------------------------------------------------------------------------------------ the reference
def sweep64(phero, walls, filt, threshold, max_val):
    """phero [C, W, H], walls [W, H], filt [S, S] -> float64 [C, W, H]: Environment.update's effect on the grid when no
    ant deposits.  Written from the definition; the oracle is not called."""
    p = np.array(phero, dtype=np.float64)
    p[:, np.asarray(walls).astype(bool)] = 0.0                      # walls.py:30  obj.phero[self.map] = 0 (update step -1)
    F = np.asarray(filt, dtype=np.float64)
    S = F.shape[0]
    R = S // 2
    C, W, H = p.shape
    pad = np.zeros((C, W + 2 * R, H + 2 * R))                       # pheromone.py:44  'fill', 0
    pad[:, R:R + W, R:R + H] = p
    out = np.zeros((C, W, H))
    for a in range(S):                                              # pheromone.py:44  convolve2d(phero, F, 'same'):
        for b in range(S):                                          #   out[x,y] = sum_{a,b} F[a,b] in[x-a+R, y-b+R]
            out += F[a, b] * pad[:, 2 * R - a:2 * R - a + W, 2 * R - b:2 * R - b + H]
    out[out < threshold] = 0.0                                      # pheromone.py:45  phero[phero < 0.01] = 0
    if max_val is not None:                                         # pheromone.py:40-41 (add_pheromones, ants.py:126-127,
        out = np.minimum(out, max_val)                              #   runs with a deposit of 0: the whole-grid minimum stays)
    return out


def sweep64_batch(phero, walls, filt, threshold, max_val):
    return np.stack([sweep64(phero[e], walls[e], filt, threshold, max_val) for e in range(phero.shape[0])])


def cfg_filter(cfg):
    S = 2 * cfg.filter_radius + 1
    return np.array(cfg.filter[:S * S], dtype=np.float64).reshape(S, S)


def cfg_max_val(cfg):
    return cfg.phero_max_val if cfg.has_max_val else None


def reference(cfg, init):
    return sweep64_batch(init["phero"], init["walls"], cfg_filter(cfg), cfg.phero_threshold, cfg_max_val(cfg))


def apriori_rtol(plan):
    """gamma_n for the kernel's own form (module docstring)."""
    S = 2 * plan["R"] + 1
    n = 1 if plan["R"] == 0 else 4 * S if plan["sep"] else 2 * S * S
    u = 2.0 ** -24
    return n * u / (1 - n * u)


# ------------------------------------------------------------------------------------------------ the plan
def filter_is_rank1(filt):
    """fill_kp (antsrl_capi.hip), the rank-1 test: F == u v^T around the largest tap, to 1e-15 of it."""
    F = np.asarray(filt, dtype=np.float64)
    S = F.shape[0]
    if S == 1:
        return False
    big, i0, j0 = 0.0, 0, 0
    for a in range(S):
        for b in range(S):
            if abs(F[a, b]) > big:
                big, i0, j0 = abs(F[a, b]), a, b
    if not big > 0.0:
        return False
    u, v = F[:, j0], F[i0, :] / F[i0, j0]
    return bool((np.abs(np.outer(u, v) - F) <= 1e-15 * big).all())


def sweep_plan(cfg):
    """launch_sweep_c (antsrl_sweep.hip:571-627) restated: which kernel runs and how it cuts the grid.  Rows x in [0, W)
    are marched in segments, columns y in [0, H) lie across the lanes in strips."""
    C, W, H, R, E = cfg.n_phero, cfg.w, cfg.h, cfg.filter_radius, cfg.n_envs
    plan = dict(C=C, W=W, H=H, R=R, E=E, sep=False, two_col=False, halo=R, seg_rows=W, nsegs=1, strip_w=H, nstrips=1)
    if R == 0:                                                      # :576
        if (W * H * C) % 4 == 0:                                    # :577
            per_env4 = W * H * C // 4                               # :578
            block = 256 * SW0_UNROLL
            plan.update(kernel="k_sweep0<%d>" % C, family="sweep0", float4_per_env=per_env4, block=block, slab=256,
                        nblocks=(per_env4 + block - 1) // block)    # :579-580
        else:
            n = E * W * H * C
            blocks = min((n + 255) // 256, SCALAR_BLOCK_CAP)        # :582-583
            plan.update(kernel="k_sweep0_scalar<%d>" % C, family="scalar", n=n, blocks=blocks,
                        passes=(n + blocks * 256 - 1) // (blocks * 256))
        return plan
    sep = filter_is_rank1(cfg_filter(cfg))
    two_col = C == 2 and H % 2 == 0                                 # :594
    seg = min(W, 16 if R == 1 else 32 if ((two_col and sep) or R == 2) else 64)  # :595
    plan.update(sep=sep, two_col=two_col, seg_rows=seg, nsegs=(W + seg - 1) // seg)  # :596
    if C == 2 and R == 1 and two_col:                               # :599-602
        plan.update(kernel="k_sweep_r1x2", family="r1x2", strip_w=128, sep=False)  # (its arithmetic is the general form's)
    elif C == 2 and R >= 2 and sep and two_col:                     # :605-611
        plan.update(kernel="k_sweep_sep2<%d>" % R, family="sep2", strip_w=128 - 4 * SEP2_HL, halo=2 * SEP2_HL)
    else:                                                           # :614-623
        plan.update(kernel="k_sweep_march<%d,%d,%d>" % (C, R, sep), family="march", strip_w=64 - 2 * R, two_col=False)
    plan["nstrips"] = (H + plan["strip_w"] - 1) // plan["strip_w"]
    return plan


def locate(plan, x, y, e=0):
    """The (strip, lane, segment) that the plan assigns output cell (x, y) of environment e, and what kind of cell it is."""
    if plan["R"] == 0:
        f = (x * plan["H"] + y) * plan["C"]
        if plan["family"] == "sweep0":                              # one grid row of workgroups per environment
            v = f // 4
            return dict(block=v // plan["block"], slab=(v % plan["block"]) // 256, float4=v)
        f += e * plan["W"] * plan["H"] * plan["C"]                  # one index space for the whole batch
        return dict(thread=f % (plan["blocks"] * 256), grid_pass=f // (plan["blocks"] * 256))
    R, ow = plan["R"], plan["strip_w"]
    strip, seg = y // ow, x // plan["seg_rows"]
    if plan["family"] == "march":
        lane = y - (strip * ow - R)                                 # :139
    elif plan["family"] == "r1x2":
        lane = (y - strip * 128) // 2                               # :314
    else:
        lane = (y - (strip * ow - 2 * SEP2_HL)) // 2                # :454
    yo, xo = y - strip * ow, x - seg * plan["seg_rows"]
    return dict(strip=strip, lane=lane, segment=seg,
                halo_neighbour=bool(yo < R or yo >= min(ow, plan["H"] - strip * ow) - R),
                overlap_row=bool(xo < R or xo >= min(plan["seg_rows"], plan["W"] - seg * plan["seg_rows"]) - R))


# ------------------------------------------------------------------------------------------------ the plan, executed
DEFECTS = ("halo_lane_dropped", "overlap_one_row_short", "last_strip_skipped_when_ragged",
           "last_segment_skipped_when_one_row", "tap_mirrored_in_y", "tap_transposed", "wall_bit_from_neighbour_word",
           "env_offset_off_by_one_cell", "second_column_of_pair_swapped", "cut_applied_before_sum",
           "grid_stride_single_pass")
_STENCIL = tuple(d for d in DEFECTS if d not in ("second_column_of_pair_swapped", "grid_stride_single_pass"))
APPLIES = {"march": _STENCIL, "r1x2": _STENCIL + ("second_column_of_pair_swapped",),
           "sep2": _STENCIL + ("second_column_of_pair_swapped",),
           "sweep0": ("last_strip_skipped_when_ragged", "wall_bit_from_neighbour_word", "env_offset_off_by_one_cell"),
           "scalar": ("wall_bit_from_neighbour_word", "env_offset_off_by_one_cell", "grid_stride_single_pass")}


def exposed(defect, plan):
    """Does the plan of this case have the seam the defect sits at?  (The others change the result on every case.)"""
    if defect == "halo_lane_dropped":       # strip 0's last halo column, y = strip_w + R - 1, lies inside the grid
        return plan["H"] >= plan["strip_w"] + plan["R"]
    if defect == "overlap_one_row_short":   # segment 0's last overlap row, x = seg_rows + R - 1, lies inside the grid
        return plan["W"] >= plan["seg_rows"] + plan["R"]
    if defect == "last_strip_skipped_when_ragged":
        if plan["family"] == "sweep0":
            return plan["float4_per_env"] % plan["block"] != 0
        return plan["H"] % plan["strip_w"] != 0
    if defect == "last_segment_skipped_when_one_row":
        return plan["W"] % plan["seg_rows"] == 1
    if defect == "grid_stride_single_pass":
        return plan["passes"] >= 2
    if defect == "env_offset_off_by_one_cell":
        return plan["E"] >= 2
    return True


def wall_words(walls):
    """uint8 [E, W, H] -> the device's bitmap: (G + 31) / 32 words per environment (fill_kp in antsrl_capi.hip), cell g in bit
    g & 31 of word g >> 5 (test_bit), environment e's words at e * words."""
    E = walls.shape[0]
    G = walls[0].size
    words = (G + 31) // 32
    bits = np.zeros((E, words * 32), np.uint8)
    bits[:, :G] = walls.reshape(E, G) != 0
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(-1).copy(), words


def _wall_bit(wbits, words, e, cell, defect):
    w = e * words + (cell >> 5)
    if defect == "wall_bit_from_neighbour_word":
        w = np.minimum(w + 1, wbits.size - 1)
    return (wbits[w] >> (cell & 31).astype(np.uint32)) & 1


def sweep_decomposed(phero, walls, filt, threshold, max_val, plan, defect=None):
    """phero [E, C, W, H], walls [E, W, H] -> float64 [E, C, W, H]: sweep64's result, unit of work by unit of work.  A
    (strip, segment) pair reads its own rows [x_lo - R, x_hi + R) and columns [y_lo - R, y_hi + R) of the device's
    cell-major buffer and its bits of the wall bitmap, and writes its own outputs.  `defect`: one of DEFECTS."""
    assert defect is None or defect in APPLIES[plan["family"]], (defect, plan["family"])
    E, C, W, H = phero.shape
    G = W * H
    dev = np.ascontiguousarray(np.asarray(phero, np.float64).transpose(0, 2, 3, 1)).reshape(E * G * C)  # [env][cell][channel]
    wbits, words = wall_words(np.asarray(walls))
    F = np.asarray(filt, np.float64)
    out = np.zeros(E * G * C)
    if plan["R"] == 0:
        def one(v):  # flat float indices -> values
            e = v // (G * C)
            cell = (v - e * G * C) // C
            src = v + (C if defect == "env_offset_off_by_one_cell" else 0) * (e > 0)
            o = dev[np.minimum(src, dev.size - 1)] * F[0, 0]
            o[o < threshold] = 0.0
            o[_wall_bit(wbits, words, e, cell, defect) != 0] = 0.0
            return o if max_val is None else np.minimum(o, max_val)
        if plan["family"] == "sweep0":
            per4, blk = plan["float4_per_env"], plan["block"]
            for e in range(E):
                for b in range(plan["nblocks"]):
                    if defect == "last_strip_skipped_when_ragged" and b == plan["nblocks"] - 1 and per4 % blk:
                        continue
                    for u in range(SW0_UNROLL):
                        v4 = b * blk + u * 256 + np.arange(256)
                        v4 = v4[v4 < per4]
                        v = (e * per4 * 4 + v4[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
                        out[v] = one(v)
        else:
            T = plan["blocks"] * 256
            for k in range(1 if defect == "grid_stride_single_pass" else plan["passes"]):
                v = k * T + np.arange(T)
                v = v[v < plan["n"]]
                out[v] = one(v)
        return out.reshape(E, W, H, C).transpose(0, 3, 1, 2)
    R, S, ow, seg = plan["R"], 2 * plan["R"] + 1, plan["strip_w"], plan["seg_rows"]
    if defect == "tap_mirrored_in_y":
        F = F[:, ::-1]
    elif defect == "tap_transposed":
        F = F.T
    out = out.reshape(E, G, C)
    dev = dev.reshape(E * G, C)
    env = np.arange(E)[:, None, None]
    base = env * G + ((env > 0) if defect == "env_offset_off_by_one_cell" else 0)        # every environment at once
    for si in range(plan["nsegs"]):
        x_lo, x_hi = si * seg, min(si * seg + seg, W)
        if defect == "last_segment_skipped_when_one_row" and si == plan["nsegs"] - 1 and x_hi - x_lo == 1:
            continue
        for st in range(plan["nstrips"]):
            y_lo, y_hi = st * ow, min(st * ow + ow, H)
            if defect == "last_strip_skipped_when_ragged" and st == plan["nstrips"] - 1 and H % ow:
                continue
            xs, ys = np.arange(x_lo - R, x_hi + R), np.arange(y_lo - R, y_hi + R)
            inside = ((xs >= 0) & (xs < W))[:, None] & ((ys >= 0) & (ys < H))[None, :]
            cell = (np.clip(xs, 0, W - 1)[:, None] * H + np.clip(ys, 0, H - 1)[None, :])[None]
            vcell = cell ^ 1 if defect == "second_column_of_pair_swapped" else cell  # (H even: a pair never wraps a row)
            tile = dev[np.minimum(base + vcell, E * G - 1)]                          # [E, rows, cols, C]
            keep = inside[None] & (_wall_bit(wbits, words, env, cell, defect) == 0)
            tile = tile * keep[..., None]
            if defect == "halo_lane_dropped":
                tile[:, :, -1, :] = 0.0
            if defect == "overlap_one_row_short":
                tile[:, -1, :, :] = 0.0
            if defect == "cut_applied_before_sum":
                tile[tile < threshold] = 0.0
            nr, nc = x_hi - x_lo, y_hi - y_lo
            acc = np.zeros((E, nr, nc, C))
            for a in range(S):
                for b in range(S):
                    acc += F[a, b] * tile[:, 2 * R - a:2 * R - a + nr, 2 * R - b:2 * R - b + nc]
            acc[acc < threshold] = 0.0
            if max_val is not None:
                acc = np.minimum(acc, max_val)
            o = (np.arange(x_lo, x_hi)[:, None] * H + np.arange(y_lo, y_hi)[None, :]).reshape(-1)
            out[:, o] = acc.reshape(E, -1, C)
    return out.reshape(E, W, H, C).transpose(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ fields and walls
FIELDS = ("dense", "near_cut", "blocks", "impulses")


def _seams(n, step):
    """Cells on both sides of every seam of an axis of n cells cut every `step`, and its two ends."""
    s = {0, n - 1}
    for k in range(step, n, step):
        s.update((k - 1, k))
    return sorted(s)


def _tile_index(plan):
    """[W, H, C] int: the unit of work that owns each float (stencils: strip + segment, the checkerboard's colour;
    radius 0: runs of 256 floats in buffer order — a wave's 64 float4, the scalar kernel's workgroup — so that the slabs
    of 256 float4 and the blocks of 1024 begin and end on a run's edge)."""
    W, H, C = plan["W"], plan["H"], plan["C"]
    if plan["R"] == 0:
        f = np.arange(W * H * C).reshape(W, H, C)
        return f // 256
    t = (np.arange(W) // plan["seg_rows"])[:, None] + (np.arange(H) // plan["strip_w"])[None, :]
    return np.broadcast_to(t[:, :, None], (W, H, C))


def _dense(rng, shape, max_val):
    n = int(np.prod(shape))
    hi = 255.0 if max_val is None else float(max_val)
    v = (1.0 + (hi - 1.0) * (rng.permutation(n) + 1.0) / n).astype(np.float32)  # (1, hi], spacing >= 6e-5 > ulp(255)
    return v.reshape(shape)


def make_field(kind, plan, max_val, seed):
    """float32 [E, C, W, H], different in every environment and channel."""
    E, C, W, H, R = plan["E"], plan["C"], plan["W"], plan["H"], plan["R"]
    rng = np.random.default_rng([seed, FIELDS.index(kind)])
    if kind == "dense":
        return _dense(rng, (E, C, W, H), max_val)
    if kind == "near_cut":
        return np.exp(rng.uniform(np.log(0.002), np.log(0.2), (E, C, W, H))).astype(np.float32)
    if kind == "blocks":
        colour = _tile_index(plan).transpose(2, 0, 1) % 2                            # [C, W, H]
        phase = (np.arange(E) % 2)[:, None, None, None]                              # env 0, 2: even tiles zero; env 1: odd
        return _dense(rng, (E, C, W, H), max_val) * ((colour[None] + phase) % 2).astype(np.float32)
    assert kind == "impulses"
    out = np.zeros((E, C, W, H), np.float32)
    gap = 2 * R + 1
    xs, ys = _seams(W, plan["seg_rows"]), _seams(H, plan["strip_w"])
    for e in range(E):
        for c in range(C):
            k = e * C + c
            cand = [(x, y) for x in (0, W - 1) for y in (0, H - 1)]                  # the corners first
            cand += [(x, (R + 1 + (i + k) * gap + 3 * k) % H) for i, x in enumerate(xs)]   # a seam row, staggered columns
            cand += [((R + 2 + (j + k) * gap + 5 * k) % W, y) for j, y in enumerate(ys)]   # a seam column, staggered rows
            cand += [(x, y) for x in xs[k % 2::2] for y in ys[(k // 2) % 2::2]]      # the seams' crossings
            taken = []
            for x, y in cand:
                if all(max(abs(x - p), abs(y - q)) >= gap for p, q in taken):
                    taken.append((x, y))
                    out[e, c, x, y] = IMPULSE
    return out


def make_walls(plan, seed, density=0.3):
    """uint8 [E, W, H]: density 0.3; environment 0 has every seam-adjacent cell walled, environment 1 none of them."""
    E, W, H = plan["E"], plan["W"], plan["H"]
    rng = np.random.default_rng([seed, 99])
    walls = (rng.random((E, W, H)) < density).astype(np.uint8)
    if plan["R"] > 0:
        seam = np.zeros((W, H), bool)
        for k in range(plan["seg_rows"], W, plan["seg_rows"]):
            seam[k - 1:k + 1, :] = True
        for k in range(plan["strip_w"], H, plan["strip_w"]):
            seam[:, k - 1:k + 1] = True
    else:
        t = _tile_index(plan)[:, :, 0]
        seam = np.zeros((W, H), bool)
        flat, tf = seam.reshape(-1), t.reshape(-1)
        edge = np.nonzero(tf[1:] != tf[:-1])[0]
        flat[edge] = True
        flat[edge + 1] = True
    if E >= 2:
        walls[0][seam] = 1
        walls[1][seam] = 0
    return walls


# ------------------------------------------------------------------------------------------------ the cases
def make_case_cfg(case, E=None, **kw):
    """The AntsCfg of a case: explicit sweep forced, four ants that never deposit unless the test says so."""
    args = dict(n_phero=case["C"], filt=case["filt"], phero_mode=cm.PHERO_EXPLICIT_SWEEP, phero_max_val=case["max_val"])
    if case["max_val"] is None:
        args["channels"] = [cm.CH_ANTS, cm.CH_WALLS]  # Pheromone(max_val=None): legal as long as no pheromone is perceived
    args.update(kw)
    return cm.make_cfg(case["E"] if E is None else E, case.get("N", 4), case["W"], case["H"], **args)


def make_init(case, cfg, field, seed=None):
    from antsrl_amd.synth import synth_init
    plan = sweep_plan(cfg)
    seed = case["seed"] if seed is None else seed
    init = synth_init(cfg, seed=seed, n_food_discs=2, food_rmin=1, food_rmax=3)
    init["walls"] = make_walls(plan, seed)
    init["food"] = init["food"] * (init["walls"] == 0)
    init["phero"] = make_field(field, plan, cfg_max_val(cfg), seed)
    return init


def _probe(C, R, filt, H):
    """The strip width and segment rows the launcher uses for this kernel, asked of sweep_plan on a large grid."""
    p = sweep_plan(cm.make_cfg(1, 1, 1000, H, n_phero=C, filt=filt, phero_mode=cm.PHERO_EXPLICIT_SWEEP))
    return p["strip_w"], p["seg_rows"], p["kernel"]


def _build_cases():
    cases = []

    def add(name, C, W, H, filt, E=3, max_val=255.0, **kw):
        case = dict(name=name, C=C, W=W, H=H, filt=filt, E=E, max_val=max_val, seed=len(cases) + 1, **kw)
        plan = sweep_plan(make_case_cfg(case))
        case.update(kernel=plan["kernel"], family=plan["family"])
        cases.append(case)
        return case

    def cross(tag, C, R, sep, parity, want):
        """H in {strip - 1, strip, strip + 1, 2 strip + 1} at W = seg + 1, W in {seg - 1, seg, seg + 1, 2 seg + 1} at
        H = strip + 1.  parity 0 / 1: the kernel needs even / odd H, and a value of the other parity takes the next one
        up (for the two-column kernels: strip, strip + 2, 2 strip + 2, and strip - 2 for the ragged single strip)."""
        filt = stencil_filter(R, sep, 10 * R + sep)
        strip, seg, kernel = _probe(C, R, filt, 1000 + (parity == 1))
        assert kernel == want, (kernel, want)

        def fix(h):
            return h if parity is None or h % 2 == parity else h + 1
        hs = sorted({fix(strip - 1) if parity != 0 else strip - 2, fix(strip), fix(strip + 1), fix(2 * strip + 1)})
        h1 = fix(strip + 1)
        shapes = [(seg + 1, h) for h in hs] + [(w, h1) for w in (seg - 1, seg, 2 * seg + 1)]
        for W, H in shapes:
            c = add("%s %dx%d" % (tag, W, H), C, W, H, filt)
            assert c["kernel"] == want, (c["name"], c["kernel"])
        big = add("%s %dx%d multi" % (tag, 2 * seg + 1, fix(2 * strip + 1)), C, 2 * seg + 1, fix(2 * strip + 1), filt,
                  multi=True)
        assert big["kernel"] == want
        if tag in ("r1x2", "sep2<3>", "march<3,2,0>"):  # Pheromone(max_val=None): one case per kernel family
            add("%s %dx%d no max_val" % (tag, seg + 1, h1), C, seg + 1, h1, filt, max_val=None)

    cross("r1x2", 2, 1, False, 0, "k_sweep_r1x2")
    cross("sep2<2>", 2, 2, True, 0, "k_sweep_sep2<2>")
    cross("sep2<3>", 2, 3, True, 0, "k_sweep_sep2<3>")
    for C in (1, 3, 4):
        for R in (1, 2, 3):
            for sep in (False, True):
                cross("march<%d,%d,%d>" % (C, R, sep), C, R, sep, None, "k_sweep_march<%d,%d,%d>" % (C, R, sep))
    for R in (1, 2, 3):       # C = 2 by way of odd H
        for sep in (False, True):
            cross("march<2,%d,%d> odd H" % (R, sep), 2, R, sep, 1, "k_sweep_march<2,%d,%d>" % (R, sep))
    for R in (2, 3):          # C = 2, even H, by way of a general filter
        cross("march<2,%d,0> even H" % R, 2, R, False, 0, "k_sweep_march<2,%d,0>" % R)
    # radius 0, explicit sweep forced.  k_sweep0<C>: float4 per environment around the slab of 256 and the block of 1024
    f0 = np.array([[0.999]])
    for C in (1, 2, 3, 4):
        for n4 in sweep0_counts(C):
            W, H = _grid_for(n4 * 4, C)
            c = add("sweep0<%d> %d float4 %dx%d" % (C, n4, W, H), C, W, H, f0, multi=(n4 == max(sweep0_counts(C))))
            assert c["kernel"] == "k_sweep0<%d>" % C, c
    add("sweep0<2> 1025 float4 no max_val", 2, _grid_for(4100, 2)[0], _grid_for(4100, 2)[1], f0, max_val=None)
    for C, W, H in ((1, 33, 35), (2, 31, 33), (3, 35, 37)):   # W H C odd, or twice an odd number (C = 4 never gets here)
        c = add("scalar<%d> %dx%d" % (C, W, H), C, W, H, f0, multi=(C == 3))
        assert c["kernel"] == "k_sweep0_scalar<%d>" % C, c
    add("scalar<1> 35x33 no max_val", 1, 35, 33, f0, max_val=None)
    # past the grid cap of 16384 workgroups x 256 threads = 4 194 304 floats: the grid-stride loop takes a second pass
    big = add("scalar<1> 129x129 x 253 envs", 1, 129, 129, f0, E=253, huge=True)
    assert sweep_plan(make_case_cfg(big))["passes"] == 2 and 253 * 129 * 129 > 4194304 > 252 * 129 * 129
    return cases


def _grid_for(floats, C):
    """W, H >= 12 with W * H * C == floats, as square as they come, or None."""
    if floats % C:
        return None
    cells, best = floats // C, None
    for w in range(12, int(cells ** 0.5) + 1):
        if cells % w == 0 and cells // w >= 12:
            best = (w, cells // w)
    return best


def sweep0_counts(C):
    """float4 per environment at the slab of 256 and the block of 256 * SW0_UNROLL: one under, on, one over.  Not every
    count is a grid: 257 is prime, so 4 * 257 floats leave no W, H >= 12 for any C, and at C = 3 the count is a
    multiple of 3.  `Under` takes the largest count below the seam that is a grid, `over` the smallest above it, `on` is
    dropped where it is none."""
    def grid(n4):
        return _grid_for(n4 * 4, C) is not None
    out = []
    for seam in (256, 256 * SW0_UNROLL):
        out.append(next(n for n in range(seam - 1, 0, -1) if grid(n)))
        if grid(seam):
            out.append(seam)
        out.append(next(n for n in range(seam + 1, 2 * seam) if grid(n)))
    return out


def in_cut_band(ref, threshold):
    """Cells of a float64 reference inside the comparator's band around the cut (helpers.CUT_BAND_RTOL)."""
    import helpers
    return np.abs(ref - threshold) <= helpers.CUT_BAND_RTOL * threshold


MULTI_STEPS = 3
_multi_cache = {}


def multi_inputs(case, field, cfg=None):
    """(nudged, init, [reference after update 1, 2, 3]) for the cases run over several updates.  A cell that the device
    puts on the other side of the cut than the reference (the comparator allows that inside its band) would rightly
    change its neighbours at the next update, so these inputs have no such cell: no reference cell lies inside the band
    after any of the updates (test_sweep_ref_cpu.py asserts it of the result).  Trying seed after seed does not get
    there at radius 3 (400 000 outputs a few of which land in a band of 8e-7 relative width under every seed), so the
    case's own field is mended instead: the non-wall input cell nearest to a cell in the band is moved by 2^-6 of its
    value, which moves every output it reaches by far more than the band, and the references are computed again."""
    key = (case["name"], field)
    if key not in _multi_cache:
        cfg = make_case_cfg(case) if cfg is None else cfg
        init = make_init(case, cfg, field)
        ph, free = init["phero"], init["walls"] == 0
        nudged = 0
        for _ in range(200):
            refs, cur = [], ph
            for _ in range(MULTI_STEPS):
                cur = sweep64_batch(cur, init["walls"], cfg_filter(cfg), cfg.phero_threshold, cfg_max_val(cfg))
                refs.append(cur)
            hits = np.argwhere(np.any([in_cut_band(r, cfg.phero_threshold) for r in refs], axis=0))
            if not len(hits):
                break
            for e, c, x, y in hits:
                fx, fy = np.nonzero(free[e] & (ph[e, c] > 0))
                k = np.argmin(np.maximum(np.abs(fx - x), np.abs(fy - y)))
                v = ph[e, c, fx[k], fy[k]]
                ph[e, c, fx[k], fy[k]] = v * np.float32(1 + 2.0 ** -6 if v < np.median(ph) else 1 - 2.0 ** -6)
                nudged += 1
        else:
            raise AssertionError("%s / %s does not leave the cut band" % key)
        _multi_cache[key] = (nudged, init, refs)
    return _multi_cache[key]


DEPOSIT_STEPS = 2


def deposit_inputs(case):
    """(cfg, init, activation or None, [(rotation, pheromone action, wall jitter)] per step): 64 ants that deposit 256 on
    top of the dense field.  They start on free cells all over the grid, the seams' neighbours among them.  Two channels:
    random pheromone actions; otherwise the activation is set directly (ants.py:86-87: activate_pheromone, :89-96,
    hard-codes two channels)."""
    cfg = make_case_cfg(dict(case, N=64), deposit_strength=256.0)
    init = make_init(case, cfg, "dense")
    rng = np.random.default_rng(case["seed"])
    E, N = cfg.n_envs, cfg.n_ants
    for e in range(E):
        fx, fy = np.nonzero(init["walls"][e] == 0)
        k = rng.choice(len(fx), N, replace=False)
        init["ants_xyt"][e, :, 0], init["ants_xyt"][e, :, 1] = fx[k] + 0.5, fy[k] + 0.5
    act = None if cfg.n_phero == 2 else rng.choice([0.0, 256.0], size=(E, N, cfg.n_phero)).astype(np.float32)
    steps = [(rng.integers(-1, 2, (E, N), dtype=np.int8),
              rng.integers(0, 3, (E, N), dtype=np.int8) if cfg.n_phero == 2 else None, rng.random((E, N)))
             for _ in range(DEPOSIT_STEPS)]
    return cfg, init, act, steps


CASES = _build_cases()
CASE_IDS = [c["name"].replace(" ", "_") for c in CASES]
FAMILIES = sorted({c["kernel"] for c in CASES})
