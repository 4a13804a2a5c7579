#!/usr/bin/env python3
"""Generates tests/golden/contract/rework_net_ref.npz by RUNNING THE REFERENCE's CollectAgentRework
(agents/collect_agent_rework.py:66-188) — build container only (the reference's checkout never travels):

    python tests/golden/make_rework_golden.py

The agent is the class as its code stands (rotations 3, pheromones 3) under torch.manual_seed(SEED), on a small reference
episode (64 ants, the generator's 6 perceived channels, main.py's All_Rewards).  Two models of `CollectModelRework`
(:24-63), each driven by the reference's own get_action(obs, agent_state, training=False) (:165-181) for STEPS steps:

  init/     the weights as constructed.  Its 20 tensors are stored whole under w/<name>.
  spread/   every .weight x W_FACTOR, every .bias x B_FACTOR, loaded into model and target_model.  At default init each
            layer shrinks its input by about 1/sqrt(3) and q is dominated by the biases: every ant takes the same action,
            which tests no argmax.  Scaled this way every action of both heads is taken by at least 5 % of the rows
            (asserted below).  Not stored: tests rebuild it from w/ and the two factors (w_factor, b_factor).

Per model and step, under <model>/: obs, agent_state, the target net's q_rot and q_ph (fp32, as torch computed them), the
returned rotation and pheromone, q64 (the same module under .double() on the same inputs, rotation head then pheromone
head) and e_ref = max |q_fp32 - q64| over the step.
Nothing of the reference's source is stored: only the arrays its code read and produced.
"""
import copy
import importlib.util
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("make_contract_golden", os.path.join(HERE, "make_contract_golden.py"))
mcg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mcg)  # its import shims + build_env (main.py's RLApi / All_Rewards, a 64 x 64 generated map)

import torch  # noqa: E402
from agents.collect_agent_rework import CollectAgentRework  # noqa: E402

SEED = 4  # the first of 1, 2, ... under which `spread` takes every action on at least 5 % of the rows (see below)
STEPS = 4
W_FACTOR = 3.0
B_FACTOR = 0.1


def run(name, rec, spread):
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(SEED)
    api, env = mcg.build_env(seed=41, n_ants=64, n_rocks=0, max_steps=STEPS + 5)
    agent = CollectAgentRework(epsilon=0.1, discount=0.5, rotations=3, pheromones=3)
    agent.setup(api, None)
    agent.initialize(api)
    if not spread:
        rec["state_dict_keys"] = np.array(list(agent.model.state_dict().keys()))
        for k, v in agent.model.state_dict().items():
            rec["w/" + k] = v.numpy().copy()
    else:
        sd = {k: v * torch.tensor(W_FACTOR if k.endswith(".weight") else B_FACTOR, dtype=torch.float32)  # an fp32 product
              for k, v in agent.model.state_dict().items()}
        agent.model.load_state_dict(sd)
        agent.target_model.load_state_dict(sd)
    model = agent.target_model
    model64 = copy.deepcopy(model).double()
    seen = {}
    fwd = model.forward

    def recording_forward(state, agent_state):
        out = fwd(state, agent_state)
        seen["q"] = out
        return out
    model.forward = recording_forward
    obs, agent_state, _ = api.observation()
    assert obs.shape[1:] == (7, 7, 6), obs.shape
    keys = ("obs", "agent_state", "q_rot", "q_ph", "rotation", "pheromone", "q64", "e_ref")
    steps = {k: [] for k in keys}
    for t in range(STEPS):
        rot, ph = agent.get_action(obs, agent_state, False)
        q_rot, q_ph = seen["q"]
        with torch.no_grad():
            q64 = torch.cat(model64(torch.Tensor(obs).double(), torch.Tensor(agent_state).double()), dim=1).numpy()
        q32 = np.concatenate([q_rot.numpy(), q_ph.numpy()], axis=1)
        e_ref = np.abs(q32.astype(np.float64) - q64).max()
        for k, v in zip(keys, (np.asarray(obs, dtype=np.float32), np.asarray(agent_state, dtype=np.float32), q_rot.numpy(),
                               q_ph.numpy(), np.asarray(rot).astype(np.int8), np.asarray(ph).astype(np.int8), q64, e_ref)):
            steps[k].append(np.asarray(v).copy())
        obs, agent_state, reward, done = api.step(rot, ph)
        env.update()
    pre = name + "/"
    for k in keys:
        rec[pre + k] = np.stack(steps[k])
    shares = [np.bincount(rec[pre + "rotation"].reshape(-1) + 1, minlength=3) / rec[pre + "rotation"].size,
              np.bincount(rec[pre + "pheromone"].reshape(-1), minlength=3) / rec[pre + "pheromone"].size]
    print(name, {k: rec[pre + k].shape for k in keys}, "e_ref", rec[pre + "e_ref"], "action shares", shares)
    if spread:
        assert min(s.min() for s in shares) >= 0.05, shares


if __name__ == "__main__":
    rec = {"seed": np.array(SEED), "w_factor": np.array(W_FACTOR, dtype=np.float32),
           "b_factor": np.array(B_FACTOR, dtype=np.float32)}
    run("init", rec, False)
    run("spread", rec, True)
    path = os.path.join(mcg.OUT, "rework_net_ref.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))
