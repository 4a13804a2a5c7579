"""The stacked-food scenario: ants of DIFFERENT WAVES standing on one food cell, step after step.

k_update_move decides every ant's mandibles from the food of its cell (RL_api.py:178-185) and then exchanges food with the
cell (ants.py:102-117): every ant reads the cell BEFORE any ant writes it, and the last ant on the cell (index order) writes.
A workgroup is one environment, a wave 64 consecutive ants.  Two ants of one cell in two waves are the case where a kernel
can get the order of the reads and the write wrong; the recordings under tests/golden have at most 64 ants (one wave) and
synth_init's states share food cells by accident only.  Here the sharing is the construction:

  * `G = min(64, N)` groups, ant i in group i % G: every group has one ant in every wave.  The ants of a group start on one
    float64 (x, y, theta) and receive one rotation per step, so they move as a stack (holding, hence speed, stays equal:
    every ant of a cell takes the same amount) until the wall jitter, which is drawn per ant, splits them.
  * food on every free cell off the anthill area, 1, 3, 5 or 2 units by (x + 2 y) % 4: with max_hold = 5 every pickup
    empties its cell, so an ant that read the cell AFTER the winner's write would see 0 and keep its mandibles open.
    (The area itself holds no food: the reference's Anthill.update empties it in every update anyway, and food there would
    make the groups that start on it close their mandibles in step 0.)
  * an anthill area of radius 3 near the centre.  Half the groups start within 1.5 cells of its centre: they leave it after
    two or more moves, so their first pickup falls into a deferred step (step 0 and step 1 run the plain k_move: the first
    update after a reset collects the whole area and is not deferred).  The other half start in a ring around the area and
    head for it: they pick up in step 0 and DROP on the area a few steps later — ants with closed mandibles on an area cell
    all drop, and one that read the cell after the winner's write would see the dropped food and stay closed.

`count_contended` counts both kinds on the oracle's state before a step, `late_read_changes_the_outcome` restates the
exchange for one cell and says whether one late read would change holding, mandibles or the cell's food — i.e. whether the
exact comparisons of tests/test_gpu_stacked_food.py would see it.  tests/test_stacked_food_cpu.py holds every case to its
floors.  Host only: numpy, and the oracle where a function is handed one."""
import numpy as np

WAVE = 64
STEPS = 24
N_ENVS, ENV_ID_BASE = 3, 5
AREA_RADIUS = 3
WALL_DENSITY = 0.03
#: the first step whose move runs inside k_update_move: update 0 collects the whole anthill area behind k_update_one and is
#: not deferred (include/antsrl.h "DEFERRED UPDATE"), so step 1 still runs k_move; update 1 is the first deferred one
FIRST_DEFERRED_STEP = 2

#: id -> (N, W, H, n_rocks, pheromone configuration)
CASES = {
    "sweep_1024_32x32": (1024, 32, 32, 0, "explicit_sweep"),
    "sweep_130_30x34": (130, 30, 34, 0, "explicit_sweep"),
    "diffuse3x3_1024_32x32": (1024, 32, 32, 0, "diffuse3x3"),
    "sweep_rocks_320_28x36": (320, 28, 36, 2, "explicit_sweep"),
    "scaled_1024_32x32": (1024, 32, 32, 0, "scaled"),
}


def case_cfg(case):
    from antsrl_amd import config as cm
    N, W, H, rocks, phero = CASES[case]
    kw = {}
    if phero == "explicit_sweep":
        kw["phero_mode"] = cm.PHERO_EXPLICIT_SWEEP
    elif phero == "diffuse3x3":
        kw["filt"] = cm.diffuse_filter(0.02, 0.001)
    cfg = cm.make_cfg(N_ENVS, N, W, H, n_rocks=rocks, act_path=cm.ACT_CELL_META, deposit_strength=256.0,
                      reward_kind=cm.REWARD_ALL, **kw)
    cfg.env_id_base = ENV_ID_BASE
    return cfg


def case_seed(case):
    """(2000: of the bases 1000, 2000, ... tried, the first that keeps every case's coordinates 5e-6 or more from an integer)"""
    return 2000 + sorted(CASES).index(case)


def stacked_init(cfg, seed):
    E, N, W, H, R = cfg.n_envs, cfg.n_ants, cfg.w, cfg.h, cfg.n_rocks
    G = min(WAVE, N)
    rng = np.random.Generator(np.random.PCG64(seed))
    xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    ants = np.empty((E, N, 3))
    walls = np.zeros((E, W, H), np.uint8)
    food = np.zeros((E, W, H), np.float32)
    xyr = np.empty((E, 3), np.int32)
    rocks = np.empty((E, R, 4)) if R else None
    group = np.arange(N) % G
    for e in range(E):
        ax, ay = W // 2 + e - 1, H // 2 + 1 - e
        xyr[e] = (ax, ay, AREA_RADIUS)
        area = (ax - xs) ** 2 + (ay - ys) ** 2 <= AREA_RADIUS ** 2
        on_area = np.arange(G) % 2 == 0
        ang = rng.random(G) * 2 * np.pi
        dist = np.where(on_area, rng.random(G) * 1.5, AREA_RADIUS + 1.5 + rng.random(G) * 2.5)
        # (the area is measured from the centre CELL's corner, anthill.py:28-33; the groups from the middle of that cell)
        cx = np.floor(ax + 0.5 + np.cos(ang) * dist).astype(int) % W
        cy = np.floor(ay + 0.5 + np.sin(ang) * dist).astype(int) % H
        gx = cx + 0.2 + 0.6 * rng.random(G)
        gy = cy + 0.2 + 0.6 * rng.random(G)
        # area groups head anywhere, ring groups towards the anthill, within 30 degrees
        to_centre = np.arctan2(ay + 0.5 - gy, ax + 0.5 - gx) + (rng.random(G) - 0.5) * (np.pi / 3)
        gt = np.where(on_area, rng.random(G) * 2 * np.pi, np.mod(to_centre, 2 * np.pi))
        wl = rng.random((W, H)) < WALL_DENSITY
        wl[area] = False
        wl[cx, cy] = False
        walls[e] = wl
        food[e] = np.where(wl | area, 0, np.array([1, 3, 5, 2])[(xs + 2 * ys) % 4])
        ants[e, :, 0], ants[e, :, 1], ants[e, :, 2] = gx[group], gy[group], gt[group]
        if R:  # one rock over the ring (it pushes whole stacks in update 0), one further out; any more sit on the second
            rocks[e] = (ax - 2.0, ay + 8.5, 3.0, 60.0)
            rocks[e, 0] = (ax + 5.5, ay + 0.5, 2.5, 80.0)
    out = dict(ants_xyt=ants, seed=rng.random((E, N)), walls=walls, food=food, anthill_xyr=xyr)
    if R:
        out["rocks"] = rocks
    return out


def stacked_actions(cfg, steps, seed):
    """-> rot[steps, E, N] (one draw per group and step), ph[steps, E, N] (one draw per ant and step), int8."""
    E, N = cfg.n_envs, cfg.n_ants
    G = min(WAVE, N)
    rng = np.random.Generator(np.random.PCG64(seed))
    rot = rng.integers(-1, 2, (steps, E, G), dtype=np.int8)[:, :, np.arange(N) % G]
    ph = rng.integers(0, 3, (steps, E, N), dtype=np.int8)
    return np.ascontiguousarray(rot), ph


def anthill_area(cfg, init):
    """[E, W, H] bool, anthill.py:28-33."""
    xs, ys = np.meshgrid(np.arange(cfg.w), np.arange(cfg.h), indexing="ij")
    a = np.asarray(init["anthill_xyr"]).reshape(cfg.n_envs, 3)
    return np.stack([np.sqrt((x - xs) ** 2 + (y - ys) ** 2) <= r for x, y, r in a])


def count_contended(oracle, cfg, init):
    """The oracle's state BEFORE a step -> (contended pickups, contended drops): two lists of cells, each a dict with the
    environment, the cell, its food, whether it lies on the area, and index / mandibles / holding of the ants on it (index
    order).  A cell counts when it holds two or more ants of two or more waves (by (int(prev_x), int(prev_y)): the cell the
    exchange uses, ants.py:102) and
      pickup: two or more of them have open mandibles, the cell is off the area and 0 < food <= max_hold
      drop:   two or more of them have closed mandibles and hold food, and the cell is on the area."""
    area = anthill_area(cfg, init)
    pickups, drops = [], []
    for e in range(cfg.n_envs):
        cx, cy = oracle.prev_x[e].astype(int), oracle.prev_y[e].astype(int)
        cell = cx * cfg.h + cy
        order = np.argsort(cell, kind="stable")
        cuts = np.nonzero(np.diff(cell[order]))[0] + 1
        for idx in np.split(order, cuts):
            if len(idx) < 2 or len(set(idx // WAVE)) < 2:
                continue
            x, y = int(cx[idx[0]]), int(cy[idx[0]])
            mand, hold = oracle.mandibles[e, idx].astype(int), oracle.holding[e, idx].copy()
            q, on_area = float(oracle.food[e, x, y]), bool(area[e, x, y])
            c = dict(env=e, x=x, y=y, food=q, on_area=on_area, idx=idx.copy(), mandibles=mand, holding=hold)
            if not on_area and 0 < q <= cfg.max_hold and (mand == 0).sum() >= 2:
                pickups.append(c)
            if on_area and ((mand == 1) & (hold > 0)).sum() >= 2:
                drops.append(c)
    return pickups, drops


def _exchange(q_read, mand, hold, on_area, max_hold):
    """ants.py:102-117 behind the mandible rule of RL_api.py:178-185 (Anthill then Food, the generator's channel order) for the
    ants of ONE cell, ant k having read q_read[k] -> (holding, mandibles, the cell's food)."""
    m = mand & (0 if on_area else 1)      # RL_api.py:184: the ant stands on the cell it exchanges with (prev == cur at a step)
    m = m | (q_read > 0)                  # :182
    closing, opening = m & (1 - mand), (1 - m) & mand
    taken = np.minimum(max_hold, np.maximum(0.0, q_read)) * closing
    dropped = hold * opening
    # ants.py:116, a fancy-index `+=`: the last ant of the cell wins, on what IT read; it is never the late reader below
    return hold + (taken - dropped), m, q_read[-1] + (dropped[-1] - taken[-1])


def late_reader(cell):
    """The position (within the cell's ants) of the ant whose late read a counted cell is probed with: the first ant that
    takes part in the contended exchange and sits in another wave than the cell's winner (its last ant); None if there is
    none."""
    idx, mand, hold = cell["idx"], cell["mandibles"], cell["holding"]
    part = (mand == 1) & (hold > 0) if cell["on_area"] else mand == 0
    for k in range(len(idx) - 1):
        if part[k] and idx[k] // WAVE != idx[-1] // WAVE:
            return k
    return None


def late_read_changes_the_outcome(food, on_area, mandibles, holding, max_hold, late):
    """One contended cell: `food` before the exchange, the ants on it in index order.  The exchange twice: every ant reads
    `food`; ant `late` (not the last one, which is the cell's winner) reads what the winner's write leaves there.  True when
    holding, mandibles or the cell's food differ between the two."""
    mand, hold = np.asarray(mandibles, int), np.asarray(holding, float)
    assert 0 <= late < len(mand) - 1
    q = np.full(len(mand), float(food))
    h0, m0, f0 = _exchange(q, mand, hold, on_area, max_hold)
    q[late] = f0
    h1, m1, f1 = _exchange(q, mand, hold, on_area, max_hold)
    return bool((h0 != h1).any() or (m0 != m1).any() or f0 != f1)


def oracle_run(case, n_threads=1):
    """The oracle driven the way tests/test_gpu_stacked_food.py drives the device -> dict(cfg, init, rot, ph, outs = the
    per-step (obs, agent_state, reward, done), contended = the per-step (pickups, drops) of count_contended, xy = every ant
    coordinate after every step and every update, oracle = the oracle after the last update)."""
    from oracle.oracle import Oracle
    cfg = case_cfg(case)
    init = stacked_init(cfg, case_seed(case))
    rot, ph = stacked_actions(cfg, STEPS, case_seed(case) + 1)
    o = Oracle(cfg, init, n_threads=n_threads)
    outs, contended, xy = [], [], [init["ants_xyt"][..., :2].copy()]
    for t in range(STEPS):
        contended.append(count_contended(o, cfg, init))
        outs.append(o.step(rot[t], ph[t]))
        xy.append(o.ants_xyt[..., :2].copy())
        o.update(None)
        xy.append(o.ants_xyt[..., :2].copy())
    return dict(cfg=cfg, init=init, rot=rot, ph=ph, outs=outs, contended=contended, xy=np.stack(xy), oracle=o)
