"""The episode renderer restated in numpy from the text of include/antsrl.h ("The episode renderer"), for
tests/test_render_ref_cpu.py, tests/test_gpu_render.py and profiles/episode_renderer_bench.py: the colour layer in
vectorised float64 (the form of the reference's mix_alpha), the composition in integers.  Plus a packer that builds a
recorder block from arrays a test chose.  Nothing here imports the product.

The frames are taken as the dictionary EpisodeRecorder.frames() / recorder_ref.decode() give: per frame [n, S, ...]
timestep, anthill_food, rock_centers, ants_xyt, holding, mandibles, reward_state, phero [n, S, C, W, H], food, explored
(absent without a heatmap); static [S, ...] anthill_xyr, rock_rw, walls."""
import numpy as np

FOOD_COLOR = (64, 255, 64)
EXPLORED_COLOR = (255, 255, 0)
ANTHILL_COLOR, ANTHILL_ALPHA = (0, 0, 255), 128
DIRT, WALL, ROCK = (134, 96, 67), (96, 96, 96), (150, 150, 150)
ANT_COLOR = np.array([255, 255, 128])
VIEW_BACKGROUND, VIEW_ANTS, VIEW_EXPLORED, VIEW_PHERO, VIEW_FOOD, VIEW_ROCKS = 1, 2, 4, 8, 16, 32
VIEW_ALL = 63
AX = np.newaxis


def mix(rgb, alpha, colour, a):
    """One layer: rgb uint8 [W, H, 3], alpha float64 [W, H]; colour at alpha a [W, H] over them."""
    fill = np.array(colour)[AX, AX, :]
    m = alpha + a * (1 - alpha)
    v = (rgb * alpha[:, :, AX] + (fill * a[:, :, AX]) * (1 - alpha[:, :, AX])) / (m[:, :, AX] + 0.001)
    return v.astype(np.uint8), m


def colour_layer(food, phero, explored, colours, phero_max_val, view=VIEW_ALL):
    """food uint8 [W, H], phero uint8 [C, W, H], explored uint8 / bool [W, H] or None -> uint8 [W, H, 4]: R, G, B and
    alpha8 of one environment of one frame."""
    rgb = np.full(food.shape + (3,), 255, dtype=np.uint8)
    alpha = np.zeros(food.shape)
    if view & VIEW_FOOD:
        rgb, alpha = mix(rgb, alpha, FOOD_COLOR, food / (float(food.max()) + 0.0001) * 0.3)
    if view & VIEW_PHERO:
        for k in range(len(phero)):
            rgb, alpha = mix(rgb, alpha, colours[k], (phero[k] / (phero_max_val + 0.0001)) * 0.6)
    if view & VIEW_EXPLORED and explored is not None:
        rgb, alpha = mix(rgb, alpha, EXPLORED_COLOR, (explored != 0) / 1.0 * 0.3)
    return np.concatenate([rgb, (alpha * 255).astype(np.uint8)[:, :, AX]], axis=2)


def blend(src, a, dst):
    """(src * a + dst * (255 - a) + 127) / 255 per channel, in integers."""
    src, a, dst = np.asarray(src, dtype=np.int64), np.asarray(a, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    return (src * a + dst * (255 - a) + 127) // 255


def compose(layer, walls, anthill_xyr, rock_centers, rock_rw, ants_xyt, holding, reward_state, zoom, view=VIEW_ALL, ant_radius=1):
    """One environment of one frame: layer uint8 [W, H, 4] -> uint8 [H * zoom, W * zoom, 3]."""
    W, H = walls.shape
    Z, ra = int(zoom), int(ant_radius)
    bg = bool(view & VIEW_BACKGROUND)
    cell = np.zeros((W, H, 3), dtype=np.int64)
    if bg:
        cell[:] = DIRT
        ax, ay, r = (int(v) for v in anthill_xyr)
        x, y = np.arange(W)[:, AX], np.arange(H)[AX, :]
        hill = (ax - x) ** 2 + (ay - y) ** 2 <= r * r
        cell[hill] = blend(ANTHILL_COLOR, ANTHILL_ALPHA, cell[hill])
    cell = blend(layer[:, :, :3], layer[:, :, 3:4], cell)
    if bg:
        cell[walls != 0] = WALL
    img = np.ascontiguousarray(cell.transpose(1, 0, 2).repeat(Z, axis=0).repeat(Z, axis=1)).astype(np.uint8)
    if view & VIEW_ROCKS:
        fx = (np.arange(W * Z) + 0.5) / Z
        fy = (np.arange(H * Z) + 0.5) / Z
        for (cx, cy), (rad, _) in zip(rock_centers, rock_rw):
            dx, dy = (fx - cx)[AX, :], (fy - cy)[:, AX]
            img[dx * dx + dy * dy <= rad * rad] = ROCK
    if view & VIEW_ANTS:
        for i in range(len(ants_xyt)):  # in index order: the highest index wins
            cx, cy = int(ants_xyt[i, 0] * Z), int(ants_xyt[i, 1] * Z)
            x0, x1 = max(cx - ra, 0), min(cx + ra + 1, W * Z)
            y0, y1 = max(cy - ra, 0), min(cy + ra + 1, H * Z)
            if x0 >= x1 or y0 >= y1:
                continue
            d2 = (np.arange(x0, x1)[AX, :] - cx) ** 2 + (np.arange(y0, y1)[:, AX] - cy) ** 2
            box = img[y0:y1, x0:x1]
            box[d2 <= ra * ra] = (ANT_COLOR * reward_state[i] / 255).astype(np.uint8)
            if holding[i] > 0:
                box[d2 <= (ra // 2) ** 2] = FOOD_COLOR
    return img


def layer_frames(f, first, count, colours, phero_max_val, view=VIEW_ALL):
    """uint8 [count, S, W, H, 4]."""
    S = f["walls"].shape[0]
    return np.stack([np.stack([colour_layer(f["food"][k, s], f["phero"][k, s], f["explored"][k, s] if "explored" in f else None,
                                            colours, phero_max_val, view) for s in range(S)]) for k in range(first, first + count)])


def render_frames(f, first, count, colours, phero_max_val, zoom, view=VIEW_ALL, ant_radius=1):
    """uint8 [count, S, H * zoom, W * zoom, 3]."""
    S = f["walls"].shape[0]
    lay = layer_frames(f, first, count, colours, phero_max_val, view)
    return np.stack([np.stack([compose(lay[k - first, s], f["walls"][s], f["anthill_xyr"][s], f["rock_centers"][k, s], f["rock_rw"][s],
                                       f["ants_xyt"][k, s], f["holding"][k, s], f["reward_state"][k, s], zoom, view, ant_radius)
                               for s in range(S)]) for k in range(first, first + count)])


def pack_block(static_fields, frame_fields, S, static, frames):
    """A recorder block from arrays.  static_fields / frame_fields: the sections [(name, dtype, shape, bytes)] of one
    environment's piece, as EpisodeRecorder exposes them (pheromone plane k is "phero%d" % k).  static: {name: [S, ...]},
    frames: {name: [n, S, ...]} with phero [n, S, C, W, H].  Returns uint8 [static_bytes + n * frame_bytes], padding zero."""
    def piece(fields, get):
        parts = []
        for name, dtype, shape, nbytes in fields:
            raw = np.ascontiguousarray(np.asarray(get(name), dtype=dtype).reshape(shape)).view(np.uint8).reshape(-1)
            parts.append(np.concatenate([raw, np.zeros(nbytes - raw.size, dtype=np.uint8)]))
        return np.concatenate(parts)

    def frame_value(k, s):
        return lambda name: frames["phero"][k, s, int(name[5:])] if name.startswith("phero") else frames[name][k, s]
    n = len(frames["food"])
    out = [piece(static_fields, lambda name, s=s: static[name][s]) for s in range(S)]
    out += [piece(frame_fields, frame_value(k, s)) for k in range(n) for s in range(S)]
    return np.concatenate(out)
