"""A caller's Reward that runs on the reference and here alike: make_probe(RewardBase) subclasses whichever `Reward` it is
given (environment/rewards/reward.py's, or antsrl_amd.rl_api.Reward) and overrides the three methods a caller overrides.
tests/golden/make_custom_reward_golden.py records it on the reference; tests/test_gpu_custom_reward.py replays it here.

What it computes (every constant dyadic and the perception used only through comparisons, so float32 versus float64
perception and any order of the sums give the same bits):

  setup        reads environment.w, environment.h and ants.n_ants only; allocates visits[n_envs, w, h] (int)
  observation  records its obs_coords; rewards = 0.125 * (unmasked perceived cells with visits == 0)
                                               + 0.5 * (unmasked cells whose Food channel is > 0)
                                               - 0.25 * (agent_state[:, 0] > 0);
               then increments visits at the unmasked coordinates (once per ant and cell)
  step         returns rewards - 0.25 * (rotation != 0)

A masked cell is -1 in every channel (RL_api.py:148) and no channel is negative otherwise, so `perception[..., 0] >= 0` is
the mask.  Food is the LAST channel (environment_generator.py:93-105, no rocks).  Row i of a folded batch belongs to env
i // (n_ants // n_envs); the reference is n_envs = 1.

make_torch_probe is the same arithmetic in torch, for RLApi(as_numpy=False): nothing leaves the device."""
import numpy as np


def make_probe(RewardBase, n_envs=1):
    class Probe(RewardBase):
        def __init__(self):
            super().__init__()
            self.visits = None
            self.seen_coords, self.seen_food, self.seen_holding = [], [], []  # what every observation() was handed

        def setup(self, ants):
            super().setup(ants)
            self.n_rows = ants.n_ants
            self.visits = np.zeros((n_envs, self.environment.w, self.environment.h), dtype=np.int64)

        def observation(self, obs_coords, perception, agent_state):
            super().observation(obs_coords, perception, agent_state)
            c = np.asarray(obs_coords)
            unmasked, food = np.asarray(perception)[..., 0] >= 0, np.asarray(perception)[..., -1] > 0
            holding = np.asarray(agent_state)[:, 0] > 0
            self.seen_coords.append(c.copy())
            self.seen_food.append(food & unmasked)
            self.seen_holding.append(holding.copy())
            self.rewards = probe_reward(self.visits, c, unmasked, food, holding)

        def step(self, done, turn_index, open_close_mandibles, on_off_pheromones):
            return self.rewards - 0.25 * (np.asarray(turn_index) != 0)

        def visualization(self):
            return (self.visits[0] > 0).astype(float)

    return Probe


def probe_reward(visits, coords, unmasked, food, holding):
    """The probe's observation() on arrays: visits int [n_envs, w, h] (updated in place), coords int [n, P, P, 2], unmasked and
    food bool [n, P, P], holding bool [n] -> float64 [n]."""
    n = coords.shape[0]
    env = np.broadcast_to((np.arange(n) // (n // visits.shape[0]))[:, None, None], unmasked.shape)
    x, y = coords[..., 0], coords[..., 1]
    fresh = (visits[env, x, y] == 0) & unmasked
    rewards = 0.125 * fresh.sum(axis=(1, 2)) + 0.5 * (food & unmasked).sum(axis=(1, 2)) - 0.25 * holding
    np.add.at(visits, (env[unmasked], x[unmasked], y[unmasked]), 1)
    return rewards


def make_torch_probe(RewardBase, n_envs=1):
    import torch

    class TorchProbe(RewardBase):
        def __init__(self):
            super().__init__()
            self.visits = None
            self.seen_coords = []

        def setup(self, ants):
            super().setup(ants)
            self.visits = None  # allocated on the first observation's device

        def observation(self, obs_coords, perception, agent_state):
            super().observation(obs_coords, perception, agent_state)
            c = obs_coords.to(torch.int64)
            self.seen_coords.append(c.clone())
            if self.visits is None:
                self.visits = torch.zeros((n_envs, self.environment.w, self.environment.h), dtype=torch.int64, device=c.device)
            n = c.shape[0]
            unmasked = perception[..., 0] >= 0
            env = (torch.arange(n, device=c.device) // (n // n_envs))[:, None, None].expand(unmasked.shape)
            x, y = c[..., 0], c[..., 1]
            fresh = (self.visits[env, x, y] == 0) & unmasked
            food = (perception[..., -1] > 0) & unmasked
            self.rewards = (0.125 * fresh.sum(dim=(1, 2)).to(torch.float64) + 0.5 * food.sum(dim=(1, 2)).to(torch.float64)
                            - 0.25 * (agent_state[:, 0] > 0).to(torch.float64))
            self.visits.index_put_((env[unmasked], x[unmasked], y[unmasked]), torch.ones((), dtype=torch.int64, device=c.device),
                                   accumulate=True)

        def step(self, done, turn_index, open_close_mandibles, on_off_pheromones):
            return self.rewards - 0.25 * (torch.as_tensor(turn_index, device=self.rewards.device) != 0).to(torch.float64)

    return TorchProbe
