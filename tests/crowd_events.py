"""Counts, from a trajectory's arrays alone, the events that the crowd fixtures (tests/golden/c*.npz, make_golden.py
crowd_scenarios) exist for: what happens to ants on the grid's edge, on wall cells, under rocks and many to a cell.

A trajectory is a dict of per-op arrays in the fixtures' layout: ops[T], ants[T,N,3], prev[T,N,2], activation[T,N,C],
rock_centers[T,R,2], plus walls[W,H], rocks[R,4] = (cx, cy, radius, weight) and deposit_strength.  A fixture gives one
(`from_fixture`), and so does an oracle run driven the way the deferred-path GPU test drives the device (`oracle_deferred_run`).

Within one Environment.update (environment.py:42-47) the order is Walls (-1), CircleObstacles (0), Ants (999), so with
`a` = the ants after the preceding op and `p` = their previous positions then:
    reverted = walls[int(a)]                       walls.py:25-27: back to prev_ants
    base     = p where reverted, else a            what CircleObstacles.update sees
    hit      = |base - centre_after| <= radius     circle_obstacles.py:53-58, with the centres it has just moved (:40)
    ants[t]  = warp(base + sum of the pushes)      ants.py:73-75
"""
import numpy as np

OP_STEP, OP_UPDATE, OP_OBSERVE = 0, 1, 2

#: event class -> the count at least one fixture (and one oracle run from a fixture's initial state) must reach
FLOORS = {
    "wraps": 100,
    "on_wall_float_activation": 20,
    "rock_centre_outside": 50,
    "inside_two_rocks": 10,
    "three_on_a_cell": 50,
    "revert_and_rock": 10,
    "push_across_edge": 1,
}


def from_fixture(F, meta, init):
    return dict(ops=F["ops"], ants=F["ants"], prev=F["prev"], activation=F["activation"], rock_centers=F["rock_centers"],
                walls=init["walls"][0].astype(bool), rocks=F["init_rocks"], deposit_strength=meta["deposit_strength"],
                init_ants=F["init_ants_xyt"])


def count_events(tr):
    ops, ants, prev, walls = tr["ops"], tr["ants"], tr["prev"], tr["walls"]
    W, H = walls.shape
    size = np.array([W, H], float)
    radius = tr["rocks"][:, 2] if len(tr["rocks"]) else np.zeros(0)
    float_act = tr["deposit_strength"] != 1.0
    n = dict.fromkeys(FLOORS, 0)
    before_xy, before_prev = tr["init_ants"][:, :2], tr["init_ants"][:, :2]
    for t, op in enumerate(ops):
        xy = ants[t][:, :2]
        if op == OP_STEP:
            # one step moves an ant by at most max_speed = 1: a jump of more than half the grid is a fold by np.mod
            n["wraps"] += int((np.abs(xy - before_xy) > size / 2).any(axis=1).sum())
        elif op == OP_UPDATE:
            cell_before = before_xy.astype(int)
            reverted = walls[cell_before[:, 0], cell_before[:, 1]]
            base = np.where(reverted[:, None], before_prev, before_xy)
            if len(radius):
                c = tr["rock_centers"][t]
                inside = np.sqrt(((c[None] - base[:, None]) ** 2).sum(-1)) <= radius[None]  # [N, R]
                n["inside_two_rocks"] += int((inside.sum(1) >= 2).sum())
                n["revert_and_rock"] += int((reverted & inside.any(1)).sum())
                n["push_across_edge"] += int((inside.any(1) & (np.abs(xy - base) > size / 2).any(axis=1)).sum())
                n["rock_centre_outside"] += int(((c[:, 0] < 0) | (c[:, 0] >= W) | (c[:, 1] < 0) | (c[:, 1] >= H)).sum())
            cell = xy.astype(int)
            if float_act:
                n["on_wall_float_activation"] += int((walls[cell[:, 0], cell[:, 1]] & (tr["activation"][t] != 0).any(1)).sum())
            _, per_cell = np.unique(cell[:, 0] * H + cell[:, 1], return_counts=True)
            n["three_on_a_cell"] += int((per_cell >= 3).sum())
        before_xy, before_prev = xy, prev[t]
    return n


def min_distance_to_integer(tr):
    """The smallest distance of any recorded ant coordinate (x or y, after any op) to an integer."""
    xy = np.concatenate([tr["ants"][..., :2].ravel(), tr["init_ants"][:, :2].ravel()])
    return float(np.abs(xy - np.round(xy)).min())


def _nudged(init):
    """The initial state with every ant's x and theta one ulp up."""
    init = dict(init)
    xyt = init["ants_xyt"].copy()
    xyt[..., 0] = np.nextafter(xyt[..., 0], np.inf)
    xyt[..., 2] = np.nextafter(xyt[..., 2], np.inf)
    init["ants_xyt"] = xyt
    return init


def oracle_replay_coordinates(cfg, init, F, meta, nudge=False):
    """The oracle replaying the recording (its ops, actions and recorded wall jitter) -> ants[T,N,3], rock_centers[T,R,2] of
    environment 0 after every op.  nudge: from the initial state moved by one ulp (the sensitivity probe)."""
    from oracle.oracle import Oracle
    o = Oracle(cfg, _nudged(init) if nudge else init)
    E = cfg.n_envs
    if meta["deposit_strength"] != 1.0:
        o.set_activation(np.broadcast_to(F["init_activation"], o.activation.shape))
    ants, rocks = [], []
    for t, op in enumerate(F["ops"]):
        if op == OP_STEP:
            o.step(np.broadcast_to(F["rot"][t], (E, cfg.n_ants)) if F["has_rot"][t] else None,
                   np.broadcast_to(F["ph"][t], (E, cfg.n_ants)) if F["has_ph"][t] else None, want_obs=False)
        elif op == OP_OBSERVE:
            o.observe(want_obs=False)
        else:
            o.update(np.broadcast_to(F["jitter"][t], (E, cfg.n_ants)))
        ants.append(o.ants_xyt[0].copy())
        rocks.append(o.rock_centers[0].copy() if cfg.n_rocks else np.zeros((0, 2)))
    return np.stack(ants), np.stack(rocks)


def oracle_deferred_run(cfg, init, F, meta, env_id_base, nudge=False, n_threads=1):
    """The oracle driven the way tests/test_gpu_crowd_deferred.py drives the device: cfg.n_envs copies of the fixture's
    initial state, its recorded actions, the library's own wall jitter keyed on env_id_base + e (so the copies diverge),
    one step + update per recorded step.  -> (per-env trajectories for count_events, per-step outputs).
    nudge: every ant's x and theta start one ulp up (the sensitivity probe)."""
    from oracle.oracle import Oracle
    cfg = cfg.copy()
    cfg.env_id_base = env_id_base
    if nudge:
        init = _nudged(init)
    o = Oracle(cfg, init, n_threads=n_threads)
    E = cfg.n_envs
    if meta["deposit_strength"] != 1.0:
        o.set_activation(np.broadcast_to(F["init_activation"], o.activation.shape))
    steps = [t for t, op in enumerate(F["ops"]) if op == OP_STEP]
    rec = dict(ops=[], ants=[], prev=[], activation=[], rock_centers=[])
    outs = []

    def keep(op):
        rec["ops"].append(op)
        rec["ants"].append(o.ants_xyt.copy())
        rec["prev"].append(np.stack([o.prev_x, o.prev_y], -1))
        rec["activation"].append(o.activation.copy())
        rec["rock_centers"].append(o.rock_centers.copy() if cfg.n_rocks else np.zeros((E, 0, 2)))

    for t in steps:
        rot = np.broadcast_to(F["rot"][t], (E, cfg.n_ants))
        ph = np.broadcast_to(F["ph"][t], (E, cfg.n_ants)) if F["has_ph"][t] else None  # (rotation-only recordings)
        outs.append(o.step(rot, ph))
        keep(OP_STEP)
        o.update(None)
        keep(OP_UPDATE)
    trs = [dict(ops=np.array(rec["ops"]), walls=init["walls"][e].astype(bool), rocks=F["init_rocks"],
                deposit_strength=meta["deposit_strength"], init_ants=F["init_ants_xyt"],
                **{k: np.stack([a[e] for a in rec[k]]) for k in ("ants", "prev", "activation", "rock_centers")})
           for e in range(E)]
    return trs, outs, o
