#!/usr/bin/env python3
"""Generates tests/golden/contract/linear_train_ref.npz by RUNNING THE REFERENCE's CollectAgent
(agents/collect_agent.py:54-184) — build container only (the reference's checkout never travels):

    python tests/golden/make_linear_train_golden.py

The agent is the class as its code stands (epsilon 0.1, discount 0.5, Adam lr 1e-4) under torch.manual_seed(SEED).  Its
initial weights are stored whole (`init/<name>`, 9 670 floats).  A small reference episode (64 ants, main.py's loop of
get_action / api.step / update_replay_memory) fills its ReplayMemory past MIN_REPLAY_MEMORY_SIZE; then CALLS train()
calls are made under a fixed random.seed, the second with done=True (UPDATE_TARGET_EVERY = 1).

Per call c, under `c<c>/`:
  idx                 the minibatch's replay indices (random.sample, replayed from the same random state)
  loss                what train() returned
  grad/<name>         p.grad just before optimizer.step, for every tensor whose .grad is not None
  delta/<name>        the parameter change of the step (after - before), all six tensors
  grad_none           the names whose .grad was None at optimizer.step (layer1)
  target_eq_model     1 if the target net's layer3 equals the model's after the call
  shared_explore      1 if model.explore_model is target_model.explore_model
The replay rows any minibatch touches are stored once (rows/...: states, agent_states, actions, rewards, new_states,
new_agent_states, dones, indexed by rows/index).  `act/`: ACT_STEPS further steps of get_action(training=False) on the
trained agent: obs, agent_state, rotation, pheromone per step, and the acting weights (the target net's) under act/w/.
The generator also checks, without storing anything, that a state_dict saved under this project's names loads into the
reference's CollectAgent.  Nothing of the reference's source is stored.
"""
import importlib.util
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("make_contract_golden", os.path.join(HERE, "make_contract_golden.py"))
mcg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mcg)  # its import shims + build_env (main.py's RLApi / All_Rewards, a 64 x 64 generated map)

import torch  # noqa: E402
from agents.collect_agent import CollectAgent  # noqa: E402

SEED = 57
FILL_STEPS = 17   # 17 x 64 ants = 1088 entries > MIN_REPLAY_MEMORY_SIZE (1000)
CALLS = 3
DONE = (False, True, False)
ACT_STEPS = 4


def main():
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(SEED)
    api, env = mcg.build_env(seed=41, n_ants=64, n_rocks=0, max_steps=FILL_STEPS + ACT_STEPS + 5)
    agent = CollectAgent(epsilon=0.1, discount=0.5, rotations=3, pheromones=3)
    agent.setup(api, None)
    agent.initialize(api)
    rec = {"seed": np.array(SEED), "discount": np.array(0.5), "lr": np.array(1e-4)}
    names = list(agent.model.state_dict().keys())
    rec["state_dict_keys"] = np.array(names)
    for k, v in agent.model.state_dict().items():
        rec["init/" + k] = v.numpy().copy()
    rec["shared_explore"] = np.array(agent.model.explore_model is agent.target_model.explore_model)

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
        seen["grad"] = {k: (None if p.grad is None else p.grad.detach().clone())
                        for k, p in agent.model.named_parameters()}
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
        none = []
        for k in names:
            g = seen["grad"][k]
            if g is None:
                none.append(k)
            else:
                rec[pre + "grad/" + k] = g.numpy().copy()
            rec[pre + "delta/" + k] = (after[k] - before[k]).numpy()
        rec[pre + "grad_none"] = np.array(none)
        tsd = agent.target_model.state_dict()
        rec[pre + "target_eq_model"] = np.array(all(torch.equal(tsd[k], after[k]) for k in names))
        print("call", c, "loss", loss, "grad None:", none, "target == model:", bool(rec[pre + "target_eq_model"]))

    rows = np.array(sorted(used))
    rec["rows/index"] = rows
    for k, v in zip(("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones"),
                    rm[rows.tolist()]):
        rec["rows/" + k] = v.numpy()

    # ---- acting: the target net, training=False
    for k, v in agent.target_model.state_dict().items():
        rec["act/w/" + k] = v.numpy().copy()
    for s in range(ACT_STEPS):
        rot, ph = agent.get_action(obs, agent_state, False)
        rec["act/s%d/obs" % s] = np.asarray(obs, dtype=np.float32).copy()
        rec["act/s%d/agent_state" % s] = np.asarray(agent_state, dtype=np.float32).copy()
        rec["act/s%d/rotation" % s] = np.asarray(rot).astype(np.int8)
        rec["act/s%d/pheromone" % s] = np.asarray(ph).astype(np.int8)
        obs, agent_state, reward, done = api.step(rot, ph)
        env.update()

    # ---- a file saved under this project's names loads into the reference's agent (checked here, nothing stored)
    sd = {k: v.clone() + 0.25 for k, v in agent.model.state_dict().items()}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "agents", "models"))
        torch.save(sd, os.path.join(tmp, "agents", "models", "roundtrip.h5"))
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            agent.load_model("roundtrip.h5")
        finally:
            os.chdir(cwd)
    assert all(torch.equal(agent.model.state_dict()[k], sd[k]) for k in names)
    assert all(torch.equal(agent.target_model.state_dict()[k], sd[k]) for k in names)
    print("load_model round trip: ok;", names)

    path = os.path.join(mcg.OUT, "linear_train_ref.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "rows", len(rows))


if __name__ == "__main__":
    main()
