#!/usr/bin/env python3
"""Generates tests/golden/contract/memory_train_ref.npz by RUNNING THE REFERENCE's CollectAgentMemory.train
(agents/collect_agent_memory.py:133-176) — build container only (the reference's checkout never travels):

    python tests/golden/make_memory_train_golden.py

The agent is the `seeded_p5` model of make_memory_golden.py: the class as its code stands (power 5, mem_size 20) under
torch.manual_seed(SEED_P5), with main.py's discount 0.99 and learning rate 1e-5.  Its weights are not stored: tests
rebuild them from the seed and check them against the stored fingerprints.  A small reference episode (64 ants,
main.py's loop of get_action / api.step / update_replay_memory, :93-105) fills its ReplayMemory past
MIN_REPLAY_MEMORY_SIZE; then CALLS train() calls are made under a fixed random.seed, the second with done=True (which
syncs the target net, UPDATE_TARGET_EVERY = 1).

Per call c, under `c<c>/`:
  idx                 the minibatch's replay indices (random.sample, replayed from the same random state)
  loss                what train() returned
  grad_fp/<name>      for the 18 tensors the loss reaches: (sum, sum of squares, first, last) of p.grad, taken just
  grad_s/<name>       before optimizer.step, and the elements at the fixed flat positions sample/<name>
  delta_fp/, delta_s/ the same for the parameter change of the step (after - before), all 26 tensors
  grad_none           the names whose .grad was None at optimizer.step (the memory head)
  target_eq_model     1 if the target net equals the model after the call
The replay rows any minibatch touches are stored once (rows/...: states, agent_states, actions, rewards, new_states,
new_agent_states, dones, indexed by rows/index).  Nothing of the reference's source is stored.
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
from agents.collect_agent_memory import CollectAgentMemory  # noqa: E402

SEED_P5 = 55
FILL_STEPS = 17   # 17 x 64 ants = 1088 entries > MIN_REPLAY_MEMORY_SIZE (1000)
CALLS = 3
DONE = (False, True, False)
N_SAMPLE = 48     # sampled elements per tensor


def fp(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([a.sum(), (a * a).sum(), a.reshape(-1)[0], a.reshape(-1)[-1]])


def main():
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(SEED_P5)
    api, env = mcg.build_env(seed=41, n_ants=64, n_rocks=0, max_steps=FILL_STEPS + 5)
    agent = CollectAgentMemory(epsilon=0.1, discount=0.99, rotations=3, pheromones=3, learning_rate=1e-5)  # main.py:53-57
    agent.setup(api, None)
    agent.initialize(api)
    rec = {"seed": np.array(SEED_P5), "discount": np.array(0.99), "lr": np.array(1e-5)}
    for k, v in agent.model.state_dict().items():
        rec["fp/" + k] = fp(v.numpy())
    names = list(agent.model.state_dict().keys())
    rec["state_dict_keys"] = np.array(names)
    rng = np.random.default_rng(7)
    sample = {k: rng.integers(0, v.numel(), N_SAMPLE) for k, v in agent.model.state_dict().items()}
    for k, s in sample.items():
        rec["sample/" + k] = s

    obs, agent_state, _ = api.observation()
    for s in range(FILL_STEPS):  # main.py:93-113, the training calls skipped below MIN_REPLAY_MEMORY_SIZE
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
                rec[pre + "grad_fp/" + k] = fp(g.numpy())
                rec[pre + "grad_s/" + k] = g.numpy().reshape(-1)[sample[k]]
            d = (after[k] - before[k]).numpy()
            rec[pre + "delta_fp/" + k] = fp(d)
            rec[pre + "delta_s/" + k] = d.reshape(-1)[sample[k]]
        rec[pre + "grad_none"] = np.array(none)
        tsd = agent.target_model.state_dict()
        rec[pre + "target_eq_model"] = np.array(all(torch.equal(tsd[k], after[k]) for k in names))
        print("call", c, "loss", loss, "grad None:", none, "target == model:", bool(rec[pre + "target_eq_model"]))

    rows = np.array(sorted(used))
    rec["rows/index"] = rows
    for k, v in zip(("states", "agent_states", "actions", "rewards", "new_states", "new_agent_states", "dones"),
                    rm[rows.tolist()]):
        rec["rows/" + k] = v.numpy()
    path = os.path.join(mcg.OUT, "memory_train_ref.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "rows", len(rows))


if __name__ == "__main__":
    main()
