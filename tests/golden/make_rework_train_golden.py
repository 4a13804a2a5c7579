#!/usr/bin/env python3
"""Generates tests/golden/contract/rework_train_ref.npz by RUNNING THE REFERENCE's CollectAgentRework
(agents/collect_agent_rework.py:66-188) — build container only (the reference's checkout never travels):

    python tests/golden/make_rework_train_golden.py

The agent is the class as its code stands (epsilon 0.1, discount 0.5, Adam lr 1e-4, rotations 3, pheromones 3) under
torch.manual_seed(SEED), make_rework_golden.py's seed and set-up: its constructed weights are asserted to equal
rework_net_ref.npz's `w/` and are not stored again.  A small reference episode (64 ants, main.py's loop of get_action /
api.step / update_replay_memory) fills its ReplayMemory past MIN_REPLAY_MEMORY_SIZE; then CALLS train() calls are made under
a fixed random.seed, the second with done=True (UPDATE_TARGET_EVERY = 1).

Per call c, under `c<c>/`:
  idx                 the minibatch's replay indices (random.sample, replayed from the same random state)
  loss, done          what train() returned, and the flag it was called with
  grad/<name>         call 0 only: p.grad just before optimizer.step, all 20 tensors
  delta/<name>        later calls: the parameter change of the step (after - before), of the ten biases and of
                      rotation_layer4.weight and pheromone_layer2.weight
  target_eq_model     1 if the target net equals the model after the call
The replay rows any minibatch touches are stored once (rows/...: states, agent_states, actions, rewards, new_states,
new_agent_states, dones, indexed by rows/index).  Nothing of the reference's source is stored.
"""
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

SEED = 4          # make_rework_golden.py's
FILL_STEPS = 17   # 17 x 64 ants = 1088 entries > MIN_REPLAY_MEMORY_SIZE (1000)
CALLS = 3
DONE = (False, True, False)


def main():
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(SEED)
    api, env = mcg.build_env(seed=41, n_ants=64, n_rocks=0, max_steps=FILL_STEPS + 5)
    agent = CollectAgentRework(epsilon=0.1, discount=0.5, rotations=3, pheromones=3)
    agent.setup(api, None)
    agent.initialize(api)
    names = list(agent.model.state_dict().keys())
    net = np.load(os.path.join(mcg.OUT, "rework_net_ref.npz"))
    assert names == list(net["state_dict_keys"])
    for k, v in agent.model.state_dict().items():
        assert np.array_equal(v.numpy(), net["w/" + k]), k
    rec = {"seed": np.array(SEED), "discount": np.array(0.5), "lr": np.array(1e-4)}

    obs, agent_state, _ = api.observation()
    for s in range(FILL_STEPS):
        action = agent.get_action(obs, agent_state, True)
        new_state, new_agent_state, reward, done = api.step(*action[:2])
        agent.update_replay_memory(obs, agent_state, action, reward, new_state, new_agent_state, done)
        obs, agent_state = new_state, new_agent_state
        env.update()
    rm = agent.replay_memory
    assert len(rm) >= 1000, len(rm)

    seen = {}
    orig_ra = rm.random_access

    def recording_random_access(n):
        st = random.getstate()
        seen["idx"] = np.array(random.sample(range(len(rm)), n))
        random.setstate(st)
        return orig_ra(n)
    rm.random_access = recording_random_access
    orig_step = agent.optimizer.step

    def recording_step(*a, **kw):
        seen["grad"] = {k: p.grad.detach().clone() for k, p in agent.model.named_parameters()}
        return orig_step(*a, **kw)
    agent.optimizer.step = recording_step

    random.seed(11)
    used = set()
    for c in range(CALLS):
        before = {k: v.clone() for k, v in agent.model.state_dict().items()}
        loss = agent.train(DONE[c], FILL_STEPS + c)
        after = agent.model.state_dict()
        pre = "c%d/" % c
        rec[pre + "idx"] = seen["idx"]
        used.update(seen["idx"].tolist())
        rec[pre + "loss"] = np.array(loss)
        rec[pre + "done"] = np.array(DONE[c])
        for k in names:
            if c == 0:
                rec[pre + "grad/" + k] = seen["grad"][k].numpy().copy()
            elif k.endswith(".bias") or k in ("rotation_layer4.weight", "pheromone_layer2.weight"):
                rec[pre + "delta/" + k] = (after[k] - before[k]).numpy()
        tsd = agent.target_model.state_dict()
        rec[pre + "target_eq_model"] = np.array(all(torch.equal(tsd[k], after[k]) for k in names))
        print("call", c, "loss", loss, "target == model:", bool(rec[pre + "target_eq_model"]))

    rows = np.array(sorted(used))
    rec["rows/index"] = rows
    for k, v in zip(("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones"),
                    rm[rows.tolist()]):
        rec["rows/" + k] = v.numpy()

    path = os.path.join(mcg.OUT, "rework_train_ref.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "rows", len(rows))


if __name__ == "__main__":
    main()
