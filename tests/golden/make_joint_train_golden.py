#!/usr/bin/env python3
"""Generates tests/golden/contract/joint_train_ref.npz by RUNNING THE REFERENCE's CollectAgent
(agents/collect_agent.py:54-184) with the freeze of layer1 lifted — build container only (the reference's checkout never
travels):

    python tests/golden/make_joint_train_golden.py

This is make_linear_train_golden.py's recording (the same seeds, the same fill episode, the same three train() calls)
with ONE difference, made here and not in the reference's sources: after agent.setup, requires_grad is set to True again
on agent.model.explore_model's parameters.  CollectModel.__init__ clears it on layer1, but CollectAgent.setup builds its
Adam over all of model.parameters(), so the reference's own train() then moves all six tensors.  Model and target net go
on sharing one ExploreModel: only layer3 has a target copy.

Per call c, under `c<c>/`:
  idx                 the minibatch's replay indices (random.sample, replayed from the same random state)
  loss                what train() returned
  grad/<name>         p.grad just before optimizer.step, for every tensor whose .grad is not None: all six
  delta/<name>        the parameter change of the step (after - before), all six tensors
  grad_none           the names whose .grad was None at optimizer.step: none
  target_eq_model     1 if the target net's state_dict equals the model's after the call
Once: shared_explore (1 if model.explore_model is target_model.explore_model, checked again after the calls), the
initial weights whole (`init/<name>`), and the replay rows any minibatch touches (rows/...: states, agent_states,
actions, rewards, new_states, new_agent_states, dones, indexed by rows/index).  No acting steps are recorded: acting is
LinearPolicy.act, held to the reference by linear_train_ref.npz.  Nothing of the reference's source is stored.
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
from agents.collect_agent import CollectAgent  # noqa: E402

SEED = 57
FILL_STEPS = 17   # 17 x 64 ants = 1088 entries > MIN_REPLAY_MEMORY_SIZE (1000)
CALLS = 3
DONE = (False, True, False)


def main():
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(SEED)
    api, env = mcg.build_env(seed=41, n_ants=64, n_rocks=0, max_steps=FILL_STEPS + 5)
    agent = CollectAgent(epsilon=0.1, discount=0.5, rotations=3, pheromones=3)
    agent.setup(api, None)
    for p in agent.model.explore_model.parameters():  # the freeze lifted: the one difference to the linear recording
        p.requires_grad = True
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

    assert agent.model.explore_model is agent.target_model.explore_model  # still one ExploreModel after the calls
    assert all(len(rec["c%d/grad_none" % c]) == 0 for c in range(CALLS))

    path = os.path.join(mcg.OUT, "joint_train_ref.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "rows", len(rows))


if __name__ == "__main__":
    main()
