"""The memory agent on the device: CollectAgentMemory (agents/collect_agent_memory.py:81-214, the agent main.py:53 runs)
with its net, its replay memory, its epsilon-greedy step and its training step all resident on the GPU.

`MemoryAgent` has the reference class's surface (setup, initialize, get_action, update_replay_memory, train, save_model,
load_model, a settable epsilon), so main.py's loop (:92-131) runs on it as it is written, and a fused form of that loop,

    rollout_step(env) = act -> select -> record_pre -> env.step_update -> record_post -> train

in which no observation is ever copied and nothing is read back to the host.  The pieces: `MemoryTrainer` (model, target
net, Adam; its `policy` is the acting target net, as :194 acts with the target net), `DeviceReplayMemory`, and the three
entries in front of antsrl_memagent.hip's kernels (antsrl_agent_select, antsrl_replay_record_pre / _post;
include/antsrl.h holds their draw specification).

What the reference stores as the "before" memory.  get_action overwrites self.previous_memory with the NEW memory
(:194) before update_replay_memory reads it (:182), so the reference stores the post-action memory in BOTH agent_states
and new_agent_states: in tests/golden/contract/memory_train_ref.npz the memory columns of rows/agent_states and
rows/new_agent_states are equal on all 621 rows.  `state_memory="reference"` (the default: parity is this project's bar)
does the same; `state_memory="carried"` stores the pre-action memory, which is what the code's shape suggests was meant.

Beyond the reference: `record_per_step` (K: how many of a step's n_envs * n_ants transitions are recorded, a stratified
sample; None = all of them, the reference's behaviour — at c3's 524 288 ants per step a ring of 50 000 rows would be
overwritten ten times per step), `replay_size`, `minibatch`, `min_replay`, `seed`, `precision` (the acting policy's),
`skip_explored` (off by default: skip the net for tiles whose ants all explore this step; results are unchanged).
Exploration is drawn once per environment and step (an environment is one reference colony).

`_LoopAgent` holds the fused loop and `initialize`, which a population of agents (population.py) runs as well;
`_DeviceAgent` adds what the single-model agents share (the hyper-parameters, the front of setup, the reference's surface
around get_action, the training state); `_InLoopAgent` adds what the two memory-less agents share on top of it: their
acting step and the bookkeeping of the in-loop policy's handle.  An agent writes its trainer, its get_action and what
it keeps between steps.  `ReworkAgent` (CollectAgentRework, the agent main.py imports first) sits on `_DeviceAgent`
directly: its net is ReworkPolicy's, and its acting step under exploration is one launch.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p
from . import config as cm
from .replay import RING_NAMES, DeviceReplayMemory
from .train import ExploreTrainer, JointTrainer, LinearTrainer, MemoryTrainer, ReworkTrainer


def _backend(api_or_env):
    """A BatchedAntsEnv, or the one behind an rl_api.RLApi."""
    b = getattr(api_or_env, "_backend", api_or_env)
    assert b is not None and hasattr(b, "step_update"), "setup needs a BatchedAntsEnv or an RLApi whose perception is set up"
    return b


class _LoopAgent:
    """The fused loop and `initialize`, for whatever acts on a BatchedAntsEnv and records into a ring: one model
    (_DeviceAgent) or a population's P (population.PopulationAgent).  A subclass has `replay_memory`, `_action_step`,
    get_action(obs, agent_state, training, env=) -> (rotation, pheromone or None[, the new memory]), train(done, step)
    and `_record_kw`, what its ring's record_pre takes by name."""

    def initialize(self, api_or_env) -> None:
        """Every pheromone activation x 10."""
        env = _backend(api_or_env)
        c = env.cfg
        env.set_activation(torch.full((c.n_envs, c.n_ants, c.n_phero), 10.0, dtype=torch.float32, device=env.device))

    def _state_memory(self):
        """The memory that goes into agent_states: none."""
        return None

    def _stepped(self, env) -> None:
        """`env` has just been stepped with this step's actions."""

    def rollout_step(self, env, training: bool = True):
        """One step of main.py's loop (:95-131) on `env` (a BatchedAntsEnv holding a current observation: after
        observe() or a step): act, select, record_pre, env.step_update (without a pheromone action when get_action gives
        none), record_post, train.  Returns the loss (0 while the replay memory is below min_replay or when not training,
        else a device tensor).  No host synchronisation: `done` for the target counter is the host's own step count
        against max_time."""
        env = _backend(env)
        obs, ast = env.obs, env.agent_state
        assert obs.is_contiguous(), "%s reads dense observation rows (obs_row_stride=None)" % type(self).__name__
        rot, ph, mem = (*self.get_action(obs, ast, training, env=env), None)[:3]
        rm = self.replay_memory
        rm.record_pre(obs, ast, self._state_memory(), rot.view(-1), None if ph is None else ph.view(-1), **self._record_kw())
        done = env.query(cm.Q_TIMESTEP) == env.cfg.max_time  # RL_api.py:200, known on the host
        shape = (env.cfg.n_envs, env.cfg.n_ants)
        env.step_update(rot.view(shape), None if ph is None else ph.view(shape))
        self._stepped(env)
        rm.record_post(env.obs, env.agent_state, mem, env.reward.view(-1), env.done)
        return self.train(done, self._action_step) if training else 0

    def run(self, env, steps: int, training: bool = True) -> list:
        """`steps` rollout_steps; the losses (device tensors, or 0) in order."""
        return [self.rollout_step(env, training) for _ in range(steps)]


class _DeviceAgent(_LoopAgent):
    """What every single-model device agent is around its get_action: the hyper-parameters, the front of setup and the
    reference's surface, on _LoopAgent's fused loop.  A subclass builds its trainer in setup, writes get_action (which
    returns (rotation, pheromone or None) and, for an agent with a memory, the new memory behind them) and overrides
    `_state_memory` when it has a memory to store and `_stepped` when it watches the environment's steps."""

    def __init__(self, name: str, epsilon: float, discount: float, rotations: int, pheromones: int, learning_rate: float,
                 record_per_step: Optional[int], replay_size: int, minibatch: int, min_replay: int,
                 update_target_every: int, seed: int):
        self.name = name
        self.epsilon, self.discount, self.rotations, self.pheromones = epsilon, discount, rotations, pheromones
        self.learning_rate = learning_rate
        self.record_per_step, self.replay_size, self.minibatch, self.min_replay = record_per_step, replay_size, minibatch, min_replay
        self.update_target_every, self.seed = update_target_every, seed
        self.trainer = self.replay_memory = self.generator = None
        self.step_counter = 0  # agent steps so far: the `step` key of the draw specification
        self._lib = _lib.load()

    def _setup(self, api_or_env, agent_states_space):
        """The front of every setup: the batch's sizes, the spaces, the replay memory (its agent_states rows
        `agent_states_space` wide), the generator and the counters.  Returns the BatchedAntsEnv."""
        env = _backend(api_or_env)
        cfg = env.cfg
        self.device = env.device
        self.n_envs, self.n_ants_per_env, self.env_id_base = cfg.n_envs, cfg.n_ants, cfg.env_id_base
        self.n_ants = cfg.n_envs * cfg.n_ants
        self.observation_space = tuple(env.obs.shape[-3:])
        self.agent_space, self.action_space = [2], [2]
        self.n_features = int(np.prod(self.observation_space))
        self.replay_memory = DeviceReplayMemory(self.replay_size, self.observation_space, agent_states_space,
                                                self.action_space, device=self.device)
        self._explored = torch.zeros((self.n_envs,), dtype=torch.uint8, device=self.device)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(self.seed)
        self.step_counter = 0
        self._action_step = 0
        return env

    def _action_buffers(self) -> None:
        """`_rot` / `_ph`: the step's actions of every ant, for an agent whose get_action returns views of its own."""
        self._rot = torch.zeros((self.n_ants,), dtype=torch.int8, device=self.device)
        self._ph = torch.zeros((self.n_ants,), dtype=torch.int8, device=self.device)

    def _select_actions(self, step: int, n_ph: int) -> None:
        """antsrl_agent_select_actions on `_rot` / `_ph`: the colonies that explore at (seed, step) take uniform actions,
        a pheromone among n_ph."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_agent_select_actions(self.seed, step, self.env_id_base, self.n_envs,
                                                             self.n_ants_per_env, float(self.epsilon), self.rotations,
                                                             n_ph, _p(self._rot), _p(self._ph), _p(self._explored),
                                                             _lib.stream(self.device)), "agent_select_actions")

    # ---- the reference's surface ----------------------------------------------------------------------------------
    @property
    def policy(self):
        return self.trainer.policy

    def _dev(self, a, dtype):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype) if (t.device != self.device or t.dtype != dtype) else t

    def _obs(self, a):
        """An observation as the kernels take it: a bfloat16 tensor as it is, anything else as float32 on the device."""
        return a if (torch.is_tensor(a) and a.dtype == torch.bfloat16) else self._dev(a, torch.float32)

    def _record_kw(self):
        return dict(n_envs=self.n_envs, n_ants=self.n_ants_per_env, k=self.record_per_step, seed=self.seed,
                    step=self._action_step, env_id_base=self.env_id_base, n_rot=self.rotations)

    def update_replay_memory(self, states, agent_state, actions, rewards, new_states, new_agent_states, done) -> None:
        """One step's transitions from arrays the caller kept (`states` must be the observation as it was BEFORE the
        step: the environment writes every observation into the same buffer).  actions = what get_action returned;
        rotation + rotations // 2 is what is stored, and 1 for a pheromone that is None (replay_memory.py:100-103)."""
        rot, ph, mem = (*actions, None)[:3]
        rm = self.replay_memory
        rm.record_pre(self._obs(states).contiguous(), self._dev(agent_state, torch.float32).contiguous(), self._state_memory(),
                      self._dev(rot, torch.int8).contiguous().view(-1),
                      None if ph is None else self._dev(ph, torch.int8).contiguous().view(-1), **self._record_kw())
        if torch.is_tensor(done) or isinstance(done, np.ndarray):
            done = self._dev(done, torch.uint8).contiguous().view(-1)
        rm.record_post(self._obs(new_states).contiguous(), self._dev(new_agent_states, torch.float32).contiguous(),
                       None if mem is None else self._dev(mem, torch.float32).contiguous(),
                       self._dev(rewards, torch.float32).contiguous().view(-1), done)

    def train(self, done: bool, step: int = 0):
        """0 below min_replay, else one step on `minibatch` rows drawn on the device; the loss stays a 0-d device
        tensor.  `done` is a host bool (the target counter lives on the host)."""
        return self.trainer.train(self.replay_memory, bool(done), minibatch=self.minibatch, min_replay=self.min_replay,
                                  generator=self.generator)

    def save_model(self, file_name: str) -> None:
        """torch.save of the model's state_dict under the reference's names (on the CPU), so the reference loads what
        this trains."""
        torch.save({k: v.cpu() for k, v in self.trainer.state_dict().items()}, file_name)

    def load_model(self, file_name: str) -> None:
        """Model and target net (and the acting policy) from a state_dict file of the reference's."""
        self.trainer.load_state_dict(torch.load(file_name, map_location="cpu"))

    # ---- the training state: out of the agent and back ------------------------------------------------------------
    #: the trainers' device buffers, whichever a trainer has: the nets (MemoryTrainer's `_model` / `_target` hold Adam's
    #: moments and the operand packs as well), Adam's moments of the flat trainers, LinearTrainer's frozen layer1
    _TRAINER_BUFFERS = ("_model", "_target", "model", "target", "heads", "target_l3", "_adam", "policy.w1", "policy.b1")
    _TRAINER_COUNTERS = ("step_count", "target_update_counter", "syncs")

    def _trainer_buffers(self) -> dict:
        out = {}
        for path in self._TRAINER_BUFFERS:
            obj = self.trainer
            for part in path.split("."):
                obj = getattr(obj, part, None)
            if torch.is_tensor(obj):
                out[path] = obj
        return out

    def training_state(self) -> dict:
        """Everything rollout_step reads or changes besides the environment, as a dict of tensors (copies, on the
        agent's device), ints, floats and bytes that torch.save takes: the trainer's nets and Adam's moments, its
        counters, the replay memory's seven tensors with head and fill, the torch generator's state, step_counter and
        `_action_step`, epsilon, `_explored`, and MemoryAgent's carried memory.  With BatchedAntsEnv.checkpoint() it is
        what a run needs to continue bit for bit (load_training_state)."""
        rm = self.replay_memory
        assert rm._pending is None, "training_state between record_pre and record_post"
        d = dict(agent=type(self).__name__, trainer={k: v.clone() for k, v in self._trainer_buffers().items()},
                 counters={k: int(getattr(self.trainer, k)) for k in self._TRAINER_COUNTERS},
                 replay={k: getattr(rm, k).clone() for k in RING_NAMES}, head=int(rm.head), fill=int(rm.fill),
                 generator=self.generator.get_state().clone(), step_counter=int(self.step_counter),
                 action_step=int(self._action_step), epsilon=float(self.epsilon), explored=self._explored.clone())
        if hasattr(self, "_mem"):  # MemoryAgent: both halves of the carried memory and which one is previous_memory
            d["memory"] = [m.clone() for m in self._mem]
            d["memory_cur"] = int(self._cur)
        return d

    def load_training_state(self, d: dict) -> None:
        """training_state()'s dict into an agent that has been set up on an env of the same shape (with the same
        hyper-parameters): every tensor is copied into the agent's own, then the acting weights are installed again (the
        trainer's acting policy, and the in-loop policy's handle where one is attached)."""
        if d["agent"] != type(self).__name__:
            raise ValueError("a %s's training state cannot go into a %s" % (d["agent"], type(self).__name__))
        tr, rm = self.trainer, self.replay_memory
        mine = self._trainer_buffers()
        pairs = [(mine.get(k), v, "trainer." + k) for k, v in d["trainer"].items()]
        pairs += [(getattr(rm, k), d["replay"][k], "replay." + k) for k in RING_NAMES]
        pairs.append((self._explored, d["explored"], "explored"))
        if hasattr(self, "_mem"):
            pairs += [(m, v, "memory") for m, v in zip(self._mem, d["memory"])]
        if set(mine) != set(d["trainer"]):
            raise ValueError("the trainer's buffers are %s, the state's %s" % (sorted(mine), sorted(d["trainer"])))
        for dst, src, what in pairs:
            if tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
                raise ValueError("%s: %s %s in the state, %s %s in this agent" % (what, src.dtype, tuple(src.shape), dst.dtype,
                                                                                 tuple(dst.shape)))
        with torch.cuda.device(self.device):
            for dst, src, _ in pairs:
                dst.copy_(src)
            self.generator.set_state(d["generator"].cpu())
        for k in self._TRAINER_COUNTERS:
            setattr(tr, k, int(d["counters"][k]))
        rm.head, rm.fill, rm._pending = int(d["head"]), int(d["fill"]), None
        self.step_counter, self._action_step, self.epsilon = int(d["step_counter"]), int(d["action_step"]), float(d["epsilon"])
        if hasattr(self, "_mem"):
            self._cur = int(d["memory_cur"])
            self._memory_before = self._mem[1 - self._cur]
        # the acting weights again: a flat trainer's acting net is views of the buffers just written (its version moves),
        # MemoryTrainer repacks its policy from the target net, ReworkTrainer collapses the target block
        if hasattr(tr, "_weights_changed"):
            tr._weights_changed()
        if hasattr(tr, "version"):
            tr.version += 1
        if hasattr(tr, "_repack_policy"):
            tr._repack_policy()
        if hasattr(tr.policy, "recollapse"):
            tr.policy.recollapse()
        self._acting_weights_loaded()

    def _acting_weights_loaded(self) -> None:
        """load_training_state has replaced the acting weights."""


class MemoryAgent(_DeviceAgent):
    """CollectAgentMemory on the device (the module docstring).  Reference lines (collect_agent_memory.py): setup
    :108-127, initialize :129-131, train :133-176, update_replay_memory :178-187, get_action :189-206, save_model
    :208-209 (the 26-tensor state_dict), load_model :211-213."""

    def __init__(self, epsilon: float = 0.1, discount: float = 0.5, rotations: int = 3, pheromones: int = 3,
                 learning_rate: float = 1e-4, *, record_per_step: Optional[int] = None, replay_size: int = 50000,
                 minibatch: int = 264, min_replay: int = 1000, update_target_every: int = 1, seed: int = 0,
                 precision: str = "bf16", state_memory: str = "reference", mem_size: int = 20, power: int = 5,
                 skip_explored: bool = False):
        assert state_memory in ("reference", "carried"), "state_memory must be 'reference' or 'carried', not %r" % (state_memory,)
        super().__init__("collect_agent_memory", epsilon, discount, rotations, pheromones, learning_rate, record_per_step,
                         replay_size, minibatch, min_replay, update_target_every, seed)
        self.precision, self.state_memory = precision, state_memory
        self.mem_size, self.power, self.skip_explored = mem_size, power, skip_explored

    def setup(self, api_or_env, trained_model: Optional[str] = None) -> None:
        """CollectAgentMemory.setup (:108-127) for every ant of the batch."""
        self.agent_and_mem_space = [2 + self.mem_size]
        self._setup(api_or_env, self.agent_and_mem_space)
        self.trainer = MemoryTrainer(self.n_features, self.device, discount=self.discount, lr=self.learning_rate,
                                     update_target_every=self.update_target_every, power=self.power, mem_size=self.mem_size,
                                     n_rot=self.rotations, n_ph=self.pheromones, seed=self.seed,
                                     policy_precision=self.precision)
        self._mem = [torch.zeros((self.n_ants, self.mem_size), dtype=torch.float32, device=self.device) for _ in range(2)]
        self._cur = 0  # self._mem[self._cur] is previous_memory (:111)
        # skip_explored: antsrl_agent_plan's list of live tiles and its length
        self._tiles = torch.zeros(((self.n_ants + 31) // 32,), dtype=torch.int32, device=self.device)
        self._n_live = torch.zeros((1,), dtype=torch.int32, device=self.device)
        if trained_model is not None:
            self.load_model(trained_model)

    @property
    def previous_memory(self) -> torch.Tensor:
        return self._mem[self._cur]

    def get_action(self, obs, agent_state, training: bool, env=None):
        """:189-206 -> (rotation int8, pheromone int8, memory float32 [M, mem_size]), device tensors.  The target net acts
        on the whole batch; with `training`, antsrl_agent_select then replaces the actions of the environments that
        explore this step (probability epsilon each) by uniform ones and gives their ants the old memory back.  With
        `skip_explored` (and `training`) antsrl_agent_plan first lists the 32-ant tiles that hold an ant of a
        non-exploring environment and the net runs on those only (antsrl_policy_memory_tiles): the same results bit for
        bit, without the forward passes select would throw away."""
        obs = self._obs(obs)
        ast = self._dev(agent_state, torch.float32)
        old, new = self._mem[self._cur], self._mem[1 - self._cur]
        step = self.step_counter
        tiles = None
        if training and self.skip_explored:
            # the net only on the tiles select leaves something of: select writes every ant of an exploring environment
            # (actions and memory), the forward every ant of a listed tile, and a tile is unlisted only when all its
            # ants explore, so every element of rot, ph and new is still written, with the bits of the full forward
            with torch.cuda.device(self.device):
                _lib.check(self._lib.antsrl_agent_plan(self.seed, step, self.env_id_base, self.n_envs, self.n_ants_per_env,
                                                       float(self.epsilon), _p(self._tiles), _p(self._n_live),
                                                       _lib.stream(self.device)), "agent_plan")
            tiles = (self._tiles, self._n_live)
        rot, ph, _ = self.policy.act(obs.contiguous(), ast.contiguous(), memory=old, out=new, env=env, tiles=tiles)
        if training:
            with torch.cuda.device(self.device):
                _lib.check(self._lib.antsrl_agent_select(self.seed, step, self.env_id_base, self.n_envs, self.n_ants_per_env,
                                                         float(self.epsilon), self.rotations, self.pheromones, self.mem_size,
                                                         _p(rot), _p(ph), _p(old), _p(new), _p(self._explored),
                                                         _lib.stream(self.device)), "agent_select")
        self._memory_before = old
        self._cur = 1 - self._cur
        self._action_step = step
        self.step_counter += 1
        return rot, ph, new

    def _state_memory(self) -> torch.Tensor:
        """The memory that goes into agent_states (see the module docstring)."""
        return self.previous_memory if self.state_memory == "reference" else self._memory_before


class _InLoopAgent(_DeviceAgent):
    """What the two memory-less agents share on top of _DeviceAgent: the acting step on a LinearPolicy and the in-loop
    form of it.  `inloop=True` takes the actions from the observation kernel (LinearPolicy.attach: bfloat16 observations
    on the cell-meta path) whenever the weights in the handle are the acting weights the observation was produced
    under, and from the standalone kernel otherwise — the two kernels give the same actions bit for bit, so both
    settings give the same actions, rings, weights and losses.  The handle's weights are refreshed
    (antsrl_set_inloop_policy) lazily: at the first step after the acting weights changed for which `_refresh_due`."""

    def __init__(self, name: str, *hyper, inloop: bool):
        super().__init__(name, *hyper)
        self.inloop = inloop
        self.inloop_hits = 0   # steps whose actions came from the observation kernel

    def _setup(self, api_or_env, agent_states_space):
        env = super()._setup(api_or_env, agent_states_space)
        # (without a pheromone head only antsrl_agent_select_actions writes _ph, the pheromone it draws for every exploring
        # ant, and nothing reads it)
        self._action_buffers()
        self._env = None            # the environment the in-loop policy is attached to
        self._handle_version = -1   # trainer.version of the weights in its handle
        self._next_version = -1     # ... of the weights its next_rotation / next_pheromone were produced under
        return env

    # ---- the in-loop policy's weights -----------------------------------------------------------------------------
    def _attach(self, env) -> None:
        self.policy.attach(env)  # allocates env.next_rotation / next_pheromone, copies the weights into the handle
        self._env, self._handle_version, self._next_version = env, self.trainer.version, -1

    def refresh_inloop(self) -> None:
        """The acting weights into the handle again (antsrl_set_inloop_policy: a 38 KB device copy and the pack; w3, b3
        and next_pheromone are None for a policy without a pheromone head)."""
        env, p = self._env, self.policy
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_set_inloop_policy(env._h, self.n_features, _p(p.w1), _p(p.b1), _p(p.w2), _p(p.b2),
                                                          _p(p.w3), _p(p.b3), _p(env.next_rotation), _p(env.next_pheromone),
                                                          _lib.stream(self.device)), "set_inloop_policy")
        self._handle_version = self.trainer.version

    def _refresh_due(self, training: bool) -> bool:
        """Whether a handle with stale weights gets the acting weights at the step that starts now."""
        raise NotImplementedError

    def _acting_weights_loaded(self) -> None:
        """The in-loop policy on the handle again (a restored env does not carry the pack), and whatever actions the
        observation kernel left are not these weights'."""
        self._next_version = -1
        if self._env is not None:
            self.refresh_inloop()

    def _stepped(self, env) -> None:
        if env is self._env:
            self._next_version = self._handle_version  # (a stale handle's actions are never equal to trainer.version)

    def get_action(self, obs, agent_state, training: bool, env=None):
        """-> (rotation int8, pheromone int8 or None), device tensors: the acting net on the whole batch (in the loop or
        standalone); with `training`, antsrl_agent_select_actions then replaces the actions of the environments that
        explore this step (probability epsilon each, one draw per environment) by uniform ones: the draws of the draw
        specification, a pheromone among 3 whether the net has that head or not."""
        obs = self._obs(obs)
        ast = self._dev(agent_state, torch.float32)
        step = self.step_counter
        lead = obs.shape[:-3]
        attached = self.inloop and env is not None and env is self._env and obs is env.obs
        if attached and self._next_version == self.trainer.version:
            rot, ph = env.next_rotation, env.next_pheromone  # what the observation kernel left for this observation
            self.inloop_hits += 1
        else:
            if attached and self._handle_version != self.trainer.version and self._refresh_due(training):
                self.refresh_inloop()
            rot, ph = self.policy.act(obs.contiguous(), ast.contiguous(), env=env)
        self._rot.copy_(rot.reshape(-1))
        if ph is not None:
            self._ph.copy_(ph.reshape(-1))
        if training:
            self._select_actions(step, 3)
        self._action_step = step
        self.step_counter += 1
        return self._rot.view(lead), (None if ph is None else self._ph.view(lead))


class CollectAgent(_InLoopAgent):
    """The linear agent on the device: CollectAgent (agents/collect_agent.py:54-184) with its net (the one config 5
    runs: LinearPolicy), its replay memory, its epsilon-greedy step and its training step resident on the GPU.

    The reference class's surface (setup, initialize, get_action, update_replay_memory, train, save_model, load_model, a
    settable epsilon) and MemoryAgent's fused loop,

        rollout_step(env) = act -> select -> record_pre -> env.step_update -> record_post -> train

    with no host synchronisation.  The pieces: `LinearTrainer` (layer2 and layer3 trained, layer1 frozen and shared with
    the target net, whose only own tensor is layer3; its `policy` is the acting net), `DeviceReplayMemory` with 2-float
    agent_states rows, and the memory-less entries antsrl_agent_select_actions / antsrl_replay_record_*_plain (the
    memory agent's kernels, draw specification and stream tags).

    `train_layer1=True` lifts the reference's freeze of layer1 and changes nothing else (the curriculum's third stage,
    DESIGN §7.21): setup builds a `JointTrainer`, whose step trains all six tensors; layer1 and layer2 stay shared with the
    target net, so every training step moves the acting weights, as it does with the freeze in place.

    `inloop=True` (_InLoopAgent): a training step changes layer2, so while the agent trains at every step the in-loop
    actions of the step before are one update old and are not used: in-loop acting pays off for the steps that do not
    train (below min_replay, training=False), and the handle is refreshed at the first step that will not train after
    the acting weights changed.

    Reference lines (collect_agent.py): setup :75-98, initialize :100-102, train :105-148, update_replay_memory
    :150-159, get_action :161-177 (the acting net is the target net: the shared layer1, the live layer2, the target
    layer3), save_model :179-180 (the six-tensor state_dict under CollectModel's names: the
    reference's CollectAgent.load_model loads it), load_model :182-184."""

    def __init__(self, epsilon: float = 0.1, discount: float = 0.5, rotations: int = 3, pheromones: int = 3,
                 learning_rate: float = 1e-4, *, record_per_step: Optional[int] = None, replay_size: int = 50000,
                 minibatch: int = 264, min_replay: int = 1000, update_target_every: int = 1, seed: int = 0,
                 inloop: bool = False, train_layer1: bool = False):
        assert rotations == 3 and pheromones == 3, "the linear net's heads are 3 wide (antsrl_policy_mlp)"
        super().__init__("collect_agent", epsilon, discount, rotations, pheromones, learning_rate, record_per_step,
                         replay_size, minibatch, min_replay, update_target_every, seed, inloop=inloop)
        self.train_layer1 = bool(train_layer1)

    def setup(self, api_or_env, trained_model: Optional[str] = None, explore_model: Optional[str] = None) -> None:
        """CollectAgent.setup (:75-98) for every ant of the batch.  `explore_model`: a four-tensor ExploreModel state_dict
        file (ExploreAgent.save_model) whose layer1 and layer2 go under the collect heads (:84, the curriculum's second
        stage: layer1 stays frozen from here on, unless `train_layer1`); applied behind `trained_model`, layer3 stays as
        it is."""
        env = self._setup(api_or_env, [2])
        trainer_cls = JointTrainer if self.train_layer1 else LinearTrainer
        self.trainer = trainer_cls(self.n_features, self.device, discount=self.discount, lr=self.learning_rate,
                                     update_target_every=self.update_target_every, seed=self.seed)
        if trained_model is not None:
            self.load_model(trained_model)
        if explore_model is not None:
            self.trainer.load_explore_state_dict(torch.load(explore_model, map_location="cpu"))
        if self.inloop:
            self._attach(env)

    def _refresh_due(self, training: bool) -> bool:
        """Only when the observation this step produces can use the weights: a step that trains moves layer2 behind
        that observation, and its in-loop actions are never taken."""
        return not self._will_train(training)

    def _will_train(self, training: bool) -> bool:
        """Whether train() at the end of the step that starts now will take a training step (it runs behind this step's
        record: the rows of this step count)."""
        k = self.n_ants if self.record_per_step is None else self.record_per_step
        return bool(training) and min(self.replay_size, len(self.replay_memory) + k) >= self.min_replay


class ExploreAgent(_InLoopAgent):
    """The explore agent on the device: ExploreAgentPytorch (agents/explore_agent_pytorch.py:48-165), the first stage of
    the curriculum whose second stage is CollectAgent (collect_agent.py:81-90 puts this net's layer1 under the collect
    heads and freezes it).  Rotation only: get_action returns (rotation, None), the environment is stepped without a
    pheromone action and the replay memory stores (rotation + 1, 1).

    The reference class cannot run as written (its forward concatenates without dim=1, :43, and train / get_action call
    the two-input model with one argument, :100, :109, :150); what is built here is what it means: ExploreModel with
    CollectModel.forward's concat (collect_agent.py:47-49) and the DQN step every other agent has, both layers trained
    and the target net a full copy (`ExploreTrainer`, antsrl_exptrain.hip).

    The surface and the fused loop are CollectAgent's.  `inloop=True` (_InLoopAgent): the acting net is the target net,
    which changes at a sync or a load only, so the handle is refreshed (without a pheromone head) at the first step
    after one of those and every other step is an in-loop hit, training or not.

    Reference lines (explore_agent_pytorch.py): setup :69-85, initialize :87-88, train :90-133, update_replay_memory
    :135-144, get_action :146-156, save_model :158-159 (the four-tensor state_dict under ExploreModel's names: the
    reference's ExploreModel loads it, and CollectAgent.setup(explore_model=...) takes it as its frozen layer1),
    load_model :162-164."""

    def __init__(self, epsilon: float = 0.1, discount: float = 0.5, rotations: int = 3, pheromones: int = 3,
                 learning_rate: float = 1e-4, *, record_per_step: Optional[int] = None, replay_size: int = 50000,
                 minibatch: int = 256, min_replay: int = 1000, update_target_every: int = 1, seed: int = 0,
                 inloop: bool = False):
        assert rotations == 3, "the net's rotation head is 3 wide (antsrl_policy_mlp)"
        super().__init__("explore_agent_pytorch", epsilon, discount, rotations, pheromones, learning_rate, record_per_step,
                         replay_size, minibatch, min_replay, update_target_every, seed, inloop=inloop)

    def setup(self, api_or_env, trained_model: Optional[str] = None) -> None:
        """ExploreAgentPytorch.setup (:69-85) for every ant of the batch."""
        env = self._setup(api_or_env, [2])
        self.trainer = ExploreTrainer(self.n_features, self.device, discount=self.discount, lr=self.learning_rate,
                                      update_target_every=self.update_target_every, seed=self.seed)
        if trained_model is not None:
            self.load_model(trained_model)
        if self.inloop:
            self._attach(env)

    def _refresh_due(self, training: bool) -> bool:
        """Always: the observation this step produces is acted on with these weights."""
        return True


class ReworkAgent(_DeviceAgent):
    """The rework agent on the device: CollectAgentRework (agents/collect_agent_rework.py:66-188, the agent main.py imports
    first) with its net (ReworkPolicy: the ten layers collapsed once per weight change), its replay memory,
    its epsilon-greedy step and its training step (ReworkTrainer, §7.15) resident on the GPU.

    The reference class's surface (setup, initialize, get_action, update_replay_memory, train, save_model, load_model, a
    settable epsilon) and _DeviceAgent's fused loop with no host synchronisation; the acting net is the target net
    (:170), so the acting weights change at a sync or a load only.  `rotations` and `pheromones` are the heads' widths,
    1 ... 8 each.

    `fused_select` (on by default): a training step acts and selects in ONE launch (ReworkPolicy.act_select,
    antsrl_policy_rework_select), which does not evaluate the net for the colonies that explore; off, it is the net on
    the whole batch and antsrl_agent_select_actions behind it.  Both give the same actions, rings, weights and losses
    bit for bit (§7.16).

    Reference lines (collect_agent_rework.py): setup :87-103, initialize :105-107, train :110-152, update_replay_memory
    :154-163, get_action :165-181, save_model :183-184 (the 20-tensor state_dict under CollectModelRework's names: the
    reference's load_model loads it), load_model :186-188."""

    def __init__(self, epsilon: float = 0.1, discount: float = 0.5, rotations: int = 3, pheromones: int = 3,
                 learning_rate: float = 1e-4, *, record_per_step: Optional[int] = None, replay_size: int = 50000,
                 minibatch: int = 264, min_replay: int = 1000, update_target_every: int = 1, seed: int = 0,
                 fused_select: bool = True):
        assert 1 <= rotations <= 8 and 1 <= pheromones <= 8, \
            "the net's heads are 1 to 8 wide (antsrl_policy_rework), not %r and %r" % (rotations, pheromones)
        super().__init__("collect_agent_rework", epsilon, discount, rotations, pheromones, learning_rate, record_per_step,
                         replay_size, minibatch, min_replay, update_target_every, seed)
        self.fused_select = fused_select

    def setup(self, api_or_env, trained_model: Optional[str] = None) -> None:
        """CollectAgentRework.setup (:87-103) for every ant of the batch."""
        self._setup(api_or_env, [2])
        self.trainer = ReworkTrainer(self.n_features, self.device, discount=self.discount, lr=self.learning_rate,
                                     update_target_every=self.update_target_every, n_rot=self.rotations,
                                     n_ph=self.pheromones, seed=self.seed)
        self._action_buffers()
        if trained_model is not None:
            self.load_model(trained_model)

    def get_action(self, obs, agent_state, training: bool, env=None):
        """:165-180 -> (rotation int8, pheromone int8), views of the agent's own buffers.  The target net acts; with
        `training` the colonies that explore this step (probability epsilon each, one draw per colony) take uniform
        actions instead, the draws of the draw specification: in the same launch (`fused_select`), or by
        antsrl_agent_select_actions behind the net."""
        obs = self._obs(obs).contiguous()
        ast = self._dev(agent_state, torch.float32).contiguous()
        step = self.step_counter
        lead = obs.shape[:-3]
        out = (self._rot, self._ph)
        if training and self.fused_select and self.epsilon > 0:
            self.policy.act_select(obs, ast, seed=self.seed, step=step, env_id_base=self.env_id_base, n_envs=self.n_envs,
                                   n_ants=self.n_ants_per_env, epsilon=self.epsilon, out=out, explored=self._explored, env=env)
        else:
            self.policy.act(obs, ast, env=env, out=out)
            if training and self.epsilon > 0:
                self._select_actions(step, self.pheromones)
        self._action_step = step
        self.step_counter += 1
        return self._rot.view(lead), self._ph.view(lead)
