"""numpy restatement of the memory agent entries of include/antsrl.h ("THE DRAW SPECIFICATION", antsrl_agent_select,
antsrl_replay_record_pre / _post), written from the header's text: the draws, epsilon-greedy select, the stratified index
and the ring rows.  The GPU tests hold the kernels to it bit for bit."""
import numpy as np

GOLD, STEP_MUL = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD1B54A32D192ED03)
DRAW_EXPLORE, DRAW_ROTATION, DRAW_PHEROMONE, DRAW_SAMPLE = (np.uint64(v) for v in (0x45584C4F, 0x524F5441, 0x50484552,
                                                                                    0x53414D50))
ONE = np.uint64(1)


def _u64(x):
    return np.atleast_1d(np.asarray(x)).astype(np.uint64)


def mix64(z):
    z = _u64(z).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def draw(seed, tag, env, step, item):
    """draw(seed, tag, env, step, item) of the header; env / item broadcast."""
    with np.errstate(over="ignore"):
        k = mix64(_u64(seed) + GOLD * (_u64(env) + ONE))
        k = mix64(k ^ (STEP_MUL * (_u64(step) + ONE)))
        k = mix64(k + GOLD * (_u64(item) + ONE))
        return mix64(k ^ tag)


def u01(k):
    return (k >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def below(k, n):
    with np.errstate(over="ignore"):
        return (((k >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def explores(seed, step, env_id_base, n_envs, epsilon):
    """bool [n_envs]: which environments explore at `step`."""
    return u01(draw(seed, DRAW_EXPLORE, env_id_base + np.arange(n_envs), step, 0)) < epsilon


def random_actions(seed, step, env_id_base, n_envs, n_ants, n_rot, n_ph):
    """(rotation, pheromone) int64 [n_envs, n_ants]: what an exploring environment's ants take."""
    env = (env_id_base + np.arange(n_envs))[:, None]
    ant = np.arange(n_ants)[None, :]
    rot = below(draw(seed, DRAW_ROTATION, env, step, ant), n_rot) - n_rot // 2
    ph = below(draw(seed, DRAW_PHEROMONE, env, step, ant), n_ph)
    return rot, ph


def select(seed, step, env_id_base, epsilon, n_rot, n_ph, rot, ph, mem_old, mem_next):
    """antsrl_agent_select on numpy arrays rot, ph [E, N], mem_old, mem_next [E, N, mem] -> (rot, ph, mem_next, explored)."""
    E, N = rot.shape
    ex = explores(seed, step, env_id_base, E, epsilon)
    r, p = random_actions(seed, step, env_id_base, E, N, n_rot, n_ph)
    return (np.where(ex[:, None], r, rot).astype(rot.dtype), np.where(ex[:, None], p, ph).astype(ph.dtype),
            np.where(ex[:, None, None], mem_old, mem_next), ex)


def sample_indices(seed, step, env_id_base, M, K):
    """a_j for j in [0, K): the ants whose transitions a step records."""
    j = np.arange(K, dtype=np.int64)
    lo, hi = j * M // K, (j + 1) * M // K
    n = hi - lo
    u = u01(draw(seed, DRAW_SAMPLE, env_id_base, step, j))
    return lo + np.minimum(np.floor(u * n.astype(np.float64)).astype(np.int64), n - 1)


def ring_rows(head, max_len, K):
    """(entries written, their ring rows, the head afterwards)."""
    js = np.arange(max(0, K - max_len), K, dtype=np.int64)
    return js, (head + js) % max_len, (head + K) % max_len
