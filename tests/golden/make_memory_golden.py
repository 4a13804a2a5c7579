#!/usr/bin/env python3
"""Generates tests/golden/contract/memory_net_ref.npz by RUNNING THE REFERENCE's memory agent — build container only
(the reference's checkout never travels):

    python tests/golden/make_memory_golden.py

Two models of `CollectModelMemory` (agents/collect_agent_memory.py:24-78), each driven by the reference's own
`CollectAgentMemory.get_action(..., training=False)` (:189-208) for 10 consecutive steps of a small reference episode
(64 ants, the generator's 6 perceived channels, main.py's All_Rewards), so the memory is carried by the reference itself:

  good_model/   the shipped checkpoint agents/models/good_model.h5 (power 4, mem_size 10).  The reference class
                hard-codes power 5, so the agent is built with mem_size 10 and its target_model's nn.Linear modules are
                replaced by ones of the checkpoint's shapes before load_state_dict; the forward that runs is the
                reference's.  Its 26 weight arrays are stored.
  seeded_p5/    the class as its code stands (power 5, mem_size 20) under torch.manual_seed(SEED_P5).  Its weights
                (1 MiB of float32) are NOT stored: tests rebuild them with torch.manual_seed and nn.Linear in the class's
                construction order, and check them against the stored per-tensor fingerprints (sum, sum of squares,
                first and last element).

Per step: obs, agent_state, memory in, q_rot, q_ph, memory out, and the actions get_action returned.
Nothing of the reference's source is stored: only the arrays its code read and produced.
"""
import importlib.util
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("make_contract_golden", os.path.join(HERE, "make_contract_golden.py"))
mcg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mcg)  # its import shims + build_env (main.py's RLApi / All_Rewards, a 64 x 64 generated map)

import torch  # noqa: E402
from torch import nn  # noqa: E402
from agents.collect_agent_memory import CollectAgentMemory  # noqa: E402

SEED_P5 = 55
STEPS = 10
LAYERS = ("layer1", "layer2", "layer3", "layer4", "rotation_layer1", "rotation_layer2", "rotation_layer3",
          "pheromone_layer1", "pheromone_layer2", "memory_layer1", "memory_layer2", "memory_layer3", "forget_layer")


def run(name, rec, checkpoint=None):
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(SEED_P5)
    api, env = mcg.build_env(seed=41, n_ants=64, n_rocks=0, max_steps=STEPS + 5)
    agent = CollectAgentMemory(epsilon=0.0, discount=0.99, rotations=3, pheromones=3, learning_rate=1e-5)  # main.py:53-57
    if checkpoint is not None:
        sd = torch.load(checkpoint, map_location="cpu")
        agent.mem_size = sd["memory_layer3.weight"].shape[0]
    agent.setup(api, None)
    agent.initialize(api)
    model = agent.target_model
    if checkpoint is not None:
        for n in LAYERS:
            out_f, in_f = sd[n + ".weight"].shape
            setattr(model, n, nn.Linear(in_f, out_f))
        model.load_state_dict(sd)
    model.eval()
    seen = {}
    fwd = model.forward

    def recording_forward(state, agent_state):
        out = fwd(state, agent_state)
        seen["q"] = out
        return out
    model.forward = recording_forward
    obs, agent_state, _ = api.observation()
    assert obs.shape[1:] == (7, 7, 6), obs.shape
    keys = ("obs", "agent_state", "mem_in", "q_rot", "q_ph", "mem_out", "a_rot", "a_ph")
    steps = {k: [] for k in keys}
    for t in range(STEPS):
        mem_in = agent.previous_memory.numpy().copy()
        rot, ph, mem_out = agent.get_action(obs, agent_state, False)
        q_rot, q_ph, new_mem = seen["q"]
        assert np.array_equal(new_mem.numpy(), mem_out)
        for k, v in zip(keys, (obs.astype(np.float32), agent_state.astype(np.float32), mem_in, q_rot.numpy(), q_ph.numpy(),
                               np.asarray(mem_out), np.asarray(rot), np.asarray(ph))):
            steps[k].append(np.asarray(v))
        obs, agent_state, reward, done = api.step(rot, ph)
        env.update()
    pre = name + "/"
    for k in keys:
        rec[pre + k] = np.stack(steps[k])
    sdm = model.state_dict()
    if checkpoint is not None:
        for k, v in sdm.items():
            rec[pre + k] = v.numpy()
    else:
        rec[pre + "seed"] = np.array(SEED_P5)
        for k, v in sdm.items():
            a = v.numpy().astype(np.float64)
            rec[pre + "fp/" + k] = np.array([a.sum(), (a * a).sum(), a.reshape(-1)[0], a.reshape(-1)[-1]])
    rec[pre + "state_dict_keys"] = np.array(list(sdm.keys()))
    print(name, {k: rec[pre + k].shape for k in keys}, "mem_size", agent.mem_size)


if __name__ == "__main__":
    rec = {}
    run("good_model", rec, os.path.join("/root/reference", "agents", "models", "good_model.h5"))
    run("seeded_p5", rec)
    path = os.path.join(mcg.OUT, "memory_net_ref.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))
