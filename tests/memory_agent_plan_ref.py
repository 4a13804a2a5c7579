"""numpy restatement of antsrl_agent_plan (include/antsrl.h), written from the header's text: the 32-ant tiles of a batch
that hold at least one ant of an environment that does not explore this step, ascending.  The explore draw is the one of
tests/memory_agent_ref.py (the header's draw specification)."""
import numpy as np

import memory_agent_ref as R

TILE = 32


def n_tiles(n_envs, n_ants):
    return -(-(n_envs * n_ants) // TILE)


def live_tiles(seed, step, env_id_base, n_envs, n_ants, epsilon):
    """int32 [n_live]: tile t = ants [32 t, min(32 t + 32, M)) of the flat [n_envs * n_ants] order is listed iff one of its
    ants belongs to an environment e with not explores(e)."""
    M, T = n_envs * n_ants, n_tiles(n_envs, n_ants)
    ant_acts = np.repeat(~R.explores(seed, step, env_id_base, n_envs, epsilon), n_ants)  # [M]: the ant's result is kept
    padded = np.zeros((T * TILE,), dtype=bool)
    padded[:M] = ant_acts
    return np.flatnonzero(padded.reshape(T, TILE).any(axis=1)).astype(np.int32)
