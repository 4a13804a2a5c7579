"""The episode recorder's block and its cast restated in numpy, from the text of include/antsrl.h ("The episode
recorder"), for tests/test_recorder_abi_cpu.py and tests/test_gpu_recorder.py.  Nothing here imports the product."""
import numpy as np


def a16(n):
    return (n + 15) // 16 * 16


def static_sections(N, W, H, C, R):
    """(name, dtype, shape, bytes) of one environment's piece of the static part, in order."""
    G = W * H
    return [("anthill_xyr", np.int32, (3,), 16), ("rock_rw", np.float64, (R, 2), 16 * R), ("walls", np.uint8, (W, H), a16(G))]


def frame_sections(N, W, H, C, R, explored):
    """(name, dtype, shape, bytes) of one environment's piece of a frame, in order (a pheromone plane is a section)."""
    G = W * H
    s = [("timestep", np.int32, (), 16), ("anthill_food", np.float64, (), 16), ("rock_centers", np.float64, (R, 2), 16 * R),
         ("ants_xyt", np.float64, (N, 3), a16(24 * N)), ("holding", np.float32, (N,), a16(4 * N)),
         ("mandibles", np.uint8, (N,), a16(N)), ("reward_state", np.uint8, (N,), a16(N))]
    s += [("phero%d" % c, np.uint8, (W, H), a16(G)) for c in range(C)]
    s.append(("food", np.uint8, (W, H), a16(G)))
    if explored:
        s.append(("explored", np.uint8, (W, H), a16(G)))
    return s


def sizes(S, N, W, H, C, R, explored, max_frames):
    """(static_bytes, frame_bytes, bytes) by the header's formulas."""
    G = W * H
    static = S * (16 + 16 * R + a16(G))
    frame = S * (32 + 16 * R + a16(24 * N) + a16(4 * N) + 2 * a16(N) + (C + 1 + (1 if explored else 0)) * a16(G))
    return static, frame, static + max_frames * frame


def section_offsets(S, N, W, H, C, R, explored, max_frames):
    """Byte offset of every section of the block: [(what, slot or (frame, slot), name, offset)]."""
    static, frame, _ = sizes(S, N, W, H, C, R, explored, max_frames)
    out = []
    for s in range(S):
        off = s * (static // S)
        for name, _, _, nbytes in static_sections(N, W, H, C, R):
            out.append(("static", s, name, off))
            off += nbytes
    for f in range(max_frames):
        for s in range(S):
            off = static + f * frame + s * (frame // S)
            for name, _, _, nbytes in frame_sections(N, W, H, C, R, explored):
                out.append(("frame", (f, s), name, off))
                off += nbytes
    return out


def decode(block, S, N, W, H, C, R, explored, n_frames):
    """block: uint8 numpy array from the block's first byte -> {name: [S, ...]} for the static fields and
    {name: [n_frames, S, ...]} for a frame's (the pheromone planes stacked as phero [n_frames, S, C, W, H])."""
    static, frame, _ = sizes(S, N, W, H, C, R, explored, 1)

    def fields(buf, sections):
        out, off = {}, 0
        for name, dtype, shape, nbytes in sections:
            used = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
            out[name] = np.ascontiguousarray(buf[..., off: off + used]).view(dtype).reshape(buf.shape[:-1] + tuple(shape))
            off += nbytes
        return out
    out = fields(block[:static].reshape(S, -1), static_sections(N, W, H, C, R))
    fr = fields(block[static: static + n_frames * frame].reshape(n_frames, S, frame // S), frame_sections(N, W, H, C, R, explored))
    fr["phero"] = np.stack([fr.pop("phero%d" % c) for c in range(C)], axis=2)
    out.update(fr)
    return out


def cast_u8(v):
    """The recorder's float32 -> uint8: truncation toward zero for 0 <= v < 256, 255 from 256 up."""
    v = np.asarray(v, dtype=np.float32)
    return np.where(v >= np.float32(256.0), 255, np.minimum(v, np.float32(255.5)).astype(np.int32)).astype(np.uint8)
