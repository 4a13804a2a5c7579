"""Populations: P agents trained in lockstep on one BatchedAntsEnv, one launch per stage of the loop whatever P is
(include/antsrl.h, "The population of linear agents" and the sections behind it).

    pop = PopulationAgent([dict(epsilon=0.5, discount=0.99, learning_rate=1e-4, seed=s) for s in range(16)],
                          record_per_step=4096, min_replay=1000)
    pop.setup(env)                      # env.cfg.n_envs = 16 * Em: member p owns environments [p Em, (p + 1) Em)
    loss = pop.rollout_step(env)        # float32 [P] on the device (0 below min_replay): five launches and the env's step

Member p is, bit for bit, the single agent run alone on a handle of its Em environments created with env_id_base =
cfg.env_id_base + p Em and the member's own seed, epsilon, discount and learning rate (tests/population_harness.py): the
kernels are the single agent's stages with the member taken from the grid, and every draw of the agents' loop is keyed
on (seed, global environment id, step).  The per-member hyper-parameters are host values that travel in the kernels'
arguments (`_Geometry.spec`): a changed epsilon costs no device copy.

The five populations, each an agent over a trainer:

    PopulationAgent         PopulationLinearTrainer    P CollectAgents, the curriculum's second stage; layer1 frozen
                                                       (antsrl_population.hip; §7.24): one training launch
    PopulationExploreAgent  PopulationExploreTrainer   P ExploreAgents, the first stage; rotation only, the acting net the
                                                       TARGET block (antsrl_popexplore.hip; §7.25): two launches
    PopulationJointAgent    PopulationJointTrainer     P CollectAgent(train_layer1=True)s, the third stage; the acting net
                                                       the LIVE block and the target layer3 (antsrl_popjoint.hip; §7.28): two
    PopulationMemoryAgent   PopulationMemoryTrainer    P MemoryAgents, the agent main.py trains; the acting net the target's
                                                       bf16 pack, the memory carried in the ring's rows behind the agent
                                                       state (antsrl_popmemtrain.hip, antsrl_popmemnet.hip; §7.29, §7.30): 17
    PopulationReworkAgent   PopulationReworkTrainer    P ReworkAgents, the agent main.py imports first; the acting net the
                                                       target block multiplied out, act and select one launch
                                                       (antsrl_poprework.hip; §7.34): four

The stages hand over device to device: `PopulationAgent.setup(env, explore_population=pop_e)`,
`PopulationJointAgent.setup(env, collect_population=pop_c)` (driver.train_population_curriculum runs them on one handle).

What is stated once:

    PopulationReplayMemory  DeviceReplayMemory's seven arrays with a leading [P]; head and fill are shared, the members
                            record the same number of rows at every step.  One call site per record half, with or without
                            a memory.
    _PopulationTrainer      the members' host values, Adam's scalars, the counters, `running_loss`, `train`, `step` (whose
                            call hands every entry the same nineteen arguments behind the net's pointers) and `workspace`.
                            A trainer holds its net's tensors, dicts and loads and names its entry (`_entry`).
    _PopulationFlatTrainer  under the explore, the joint and the rework trainer, train._FlatTrainer's counterpart: a member's net is
                            one flat block; the name table, `_sizes`, `_views`, `adam_state`, Adam's tensor, `grads`, `_entry`.
    _Population             the members' host values, the front of setup, the step's one AntsPopSpec, `get_action`, the
                            ring, train, the fused loop, the per-member files, `exploit` (every pair and per-member array
                            in one launch, antsrl_pop_exploit; antsrl_amd/pbt.py) and `copy_member`.  An agent names its
                            trainer class and launches its acting net (`_policy`); the memory agent also has its own
                            select and hands its new memory out behind the actions.

Out of scope: the memory agents' explore plan and tile-list forward (skip_explored) and their fp32 acting precision;
in-loop acting (a handle holds one policy pack), B > 512 for the
linear nets, members of unequal size, training_state.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p
from .agent import _LoopAgent, _backend
from .policy import (MEMNET_PRECISIONS, REWORK_LAYERS, linear_init, memnet_param_ptrs, memnet_param_shapes, memnet_shape,
                     rework_param_shapes)
from .replay import RING_NAMES, _Ring, ring_arrays
from .train import (EXPLORE_NAMES, LINEAR_NAMES, _MemoryBlocks, _TargetCounter, _clones, collect_names, copy_named,
                    explore_names, linear_adam_state, linear_model_views, linear_target_state_dict)

MEMBER_DEFAULTS = dict(epsilon=0.1, discount=0.5, learning_rate=1e-4, seed=0)  # CollectAgent's


def _members(members: Sequence[dict]) -> list:
    assert 1 <= len(members) <= _lib.POP_MAX, "a population has 1 .. %d members (%d)" % (_lib.POP_MAX, len(members))
    out = []
    for m in members:
        extra = set(m) - set(MEMBER_DEFAULTS)
        assert not extra, "a member is dict(epsilon=, discount=, learning_rate=, seed=), not %s" % sorted(extra)
        out.append(dict(MEMBER_DEFAULTS, **m))
    return out


def _rows(p: Optional[int]) -> slice:
    """Member p, or every member (None): the rows of a [P, ...] tensor, and range(P)[rows] the members themselves."""
    return slice(None) if p is None else slice(p, p + 1 or None)


class _Geometry:
    """What every entry's AntsPopSpec says of the handle: the batch, the observation rows and the members' host values."""

    def __init__(self, n_members: int, n_envs: int, n_ants: int, env_id_base: int, n_features: int, obs_dtype):
        if n_envs % n_members:
            raise ValueError("n_envs = %d is not a multiple of the population's %d members" % (n_envs, n_members))
        self.P, self.n_envs, self.n_ants, self.env_id_base, self.n_features = n_members, n_envs, n_ants, env_id_base, n_features
        self.Em = n_envs // n_members
        self.Mm = self.Em * n_ants
        self.obs_format = 1 if obs_dtype == torch.bfloat16 else 0  # ANTSRL_OBS_BF16 / ANTSRL_OBS_F32

    def spec(self, seed, epsilon, learning_rate, discount) -> _lib.AntsPopSpec:
        """The AntsPopSpec of these host values.  The last one built is kept and handed out again while the values stay
        the same: a step builds none, an episode's new epsilons build one."""
        key = (tuple(int(v) for v in seed), tuple(float(v) for v in epsilon), tuple(float(v) for v in learning_rate),
               tuple(float(v) for v in discount))
        if getattr(self, "_spec_key", None) != key:
            s = _lib.AntsPopSpec(self.P, self.n_envs, self.n_ants, self.env_id_base, self.n_features, self.obs_format, 0, 0)
            for p in range(self.P):
                s.members[p] = _lib.AntsPopMember(key[0][p], key[1][p], key[2][p], key[3][p], 0)
            self._spec_key, self._spec = key, s
        return self._spec


class _MemberRing:
    """Member p's slab of a PopulationReplayMemory under DeviceReplayMemory's names (views, not copies)."""

    def __init__(self, ring, p: int):
        for n in RING_NAMES:
            setattr(self, n, getattr(ring, n)[p])
        self.head, self.fill, self.max_len = ring.head, ring.fill, ring.max_len

    def __len__(self):
        return self.fill


class PopulationReplayMemory(_Ring):
    """DeviceReplayMemory's seven arrays with a leading [P]: states [P, max_len, 7, 7, K] and so on.  `head` and `fill`
    are shared.  record_pre / record_post are antsrl_pop_record_pre / _post: K rows per member and step into the same
    rows of every member's slab, each member sampling its own ants with its own seed.  They take their tensors in the
    order DeviceReplayMemory's do and the step's AntsPopSpec, step and k by name.  agent_states_space: a row of
    agent_states and new_agent_states, (2,) for the linear nets (memory: None, those agents have none); the ring a
    PopulationMemoryTrainer steps on has (2 + mem_size,): its record halves take `memory` (float32 [M, mem_size], every
    member's rows) and, by name, the net's `shape`, and are antsrl_pop_memory_record_pre / _post."""

    def __init__(self, n_members: int, max_len: int, observation_space: Sequence[int], device="cuda",
                 agent_states_space: Sequence[int] = (2,)):
        self.n_members, self.observation_space = n_members, tuple(observation_space)
        self._alloc(max_len, observation_space, list(agent_states_space), [2], device, lead=(n_members,))
        self.mem_size = int(np.prod(agent_states_space)) - 2  # what a row carries behind the agent state

    def member(self, p: int) -> _MemberRing:
        """Member p's slab under DeviceReplayMemory's seven names, with head and fill (views: same_rings works on it)."""
        return _MemberRing(self, p)

    def _memory(self, memory, shape) -> None:
        """A memory (and the net's shape) exactly when the rows are wider than the agent state."""
        if self.mem_size == 0:
            assert memory is None, "a population's agents have no memory"
            return
        assert shape is not None and shape.mem_size == self.mem_size, "a ring with a memory records with the net's shape"
        assert memory is not None and memory.dtype == torch.float32 and memory.is_contiguous() and \
            memory.shape[-1] == self.mem_size, "memory: float32 [M, %d]" % self.mem_size

    def _record(self, half: str, pending: tuple, obs, agent_state, memory, rest: tuple) -> None:
        """antsrl_pop_record_<half> on (spec, step, k, shape) = pending: the step's rows, then `rest` (the half's other
        inputs and the ring's arrays it writes).  A ring with a memory puts the shape behind the spec and the memory
        behind the agent state, and calls antsrl_pop_memory_record_<half>."""
        spec, step, k, shape = pending
        self._memory(memory, shape)
        name = ("pop_memory_record_" if self.mem_size else "pop_record_") + half
        lead, mem = ((C.byref(spec), C.byref(shape)), (_p(memory),)) if self.mem_size else ((C.byref(spec),), ())
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), "antsrl_" + name)(*lead, step, k, self.head, self.max_len, _p(obs), _p(agent_state),
                                                              *mem, *map(_p, rest), _lib.stream(self.device)), name)

    def record_pre(self, obs, agent_state, memory, rotation, pheromone, *, spec, step: int, k: int, shape=None) -> None:
        """Before the environment step: states, agent_states and actions of k of every member's transitions."""
        assert self._pending is None, "record_pre twice without record_post"
        self._record("pre", (spec, step, k, shape), obs, agent_state, memory,
                     (rotation, pheromone, self.states, self.agent_states, self.actions))
        self._pending = (spec, step, k, shape)

    def record_post(self, obs, agent_state, memory, reward, done) -> None:
        """After it: rewards, new_states, new_agent_states and dones of the same transitions; then head and fill advance
        as DeviceReplayMemory's do for k rows."""
        assert self._pending is not None, "record_post without record_pre"
        if done.dtype == torch.bool:
            done = done.view(torch.uint8)
        self._record("post", self._pending, obs, agent_state, memory,
                     (reward, done, self.rewards, self.new_states, self.new_agent_states, self.dones.view(torch.uint8)))
        k = self._pending[2]
        self._pending = None
        self._advance(k)


class _PopulationTrainer(_TargetCounter):
    """What the population trainers share.  Per member: seed, discount and learning rate.  Common: Adam's betas, eps
    and step count, update_target_every and the target counter.  `running_loss` (float64 [P]) is main.py:106-109's
    running loss per member, kept by the training step's last launch from the first training step on.  `_spec`, `train`,
    `step` and `workspace` are here; a subclass allocates its tensors (`grads` among them), holds the dict and load
    methods of its net, names its entry (`_entry`) and says how large the step's workspace is (`_workspace_bytes`)."""

    def __init__(self, geometry: _Geometry, device, seeds, discount, lr, betas, eps: float, update_target_every: int):
        self.g, self.device = geometry, torch.device(device)
        self.n_members, self.n_features = geometry.P, geometry.n_features
        self.seeds = [int(s) for s in seeds]
        self.discount, self.lr = np.asarray(discount, dtype=np.float64).copy(), np.asarray(lr, dtype=np.float64).copy()
        self.betas, self.eps, self.update_target_every = tuple(float(b) for b in betas), float(eps), int(update_target_every)
        self.target_update_counter = self.syncs = self.step_count = 0
        self.running_loss = torch.zeros((self.n_members,), dtype=torch.float64, device=self.device)
        self.last_idx = None  # the [P, B] indices of the last step
        self._work, self._work_B = None, 0
        self._lib = _lib.load()

    def _spec(self):
        """The spec of a step driven without an agent (epsilon 0: the training entry reads none)."""
        return self.g.spec(self.seeds, np.zeros(self.n_members), self.lr, self.discount)

    def _entry(self) -> tuple:
        """(the training entry, its name in an error, the net's pointers that lead its arguments)."""
        raise NotImplementedError

    def _workspace_bytes(self, B: int) -> Optional[int]:
        """The bytes of the step's workspace for B rows per member (the entry's _sizes says); None: the step has none."""
        raise NotImplementedError

    def workspace(self, B: int) -> Optional[torch.Tensor]:
        """The step's workspace for B rows per member (uint8, 256-byte aligned; member p's part starts p strides in),
        allocated when B changes and handed to the entry behind first_loss; None for a step without one."""
        if self._work_B != B:
            n = self._workspace_bytes(B)
            self._work = None if n is None else torch.empty((n,), dtype=torch.uint8, device=self.device)
            self._work_B = B
        return self._work

    def step(self, ring: PopulationReplayMemory, idx: torch.Tensor, spec=None, loss: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step of every member on its rows idx[p] (int64 [P, B] on the device, values in [0, fill)) of its
        slab: gradient, loss and Adam in the entry's launches, whatever P is.  Returns the losses, float32 [P] on the
        device.  spec: the agent's AntsPopSpec of this step (its seeds, learning rates and discounts are this trainer's),
        else one is built.  loss: where the losses go (as the single trainers' step takes it), else a new tensor."""
        P = self.n_members
        assert idx.device == self.device and idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[0] == P and idx.is_contiguous()
        if loss is None:
            loss = torch.empty((P,), dtype=torch.float32, device=self.device)
        assert loss.device == self.device and loss.dtype == torch.float32 and loss.shape == (P,) and loss.is_contiguous()
        entry, who, net = self._entry()
        work = self.workspace(idx.shape[1])
        tail = () if work is None else (_p(work),)
        first = self.step_count == 0
        self.step_count += 1
        with torch.cuda.device(self.device):
            _lib.check(entry(C.byref(self._spec() if spec is None else spec), *net, *map(_p, ring_arrays(ring)), ring.max_len,
                             _p(idx), idx.shape[1], self.step_count, self.betas[0], self.betas[1], self.eps, _p(self.grads),
                             _p(loss), _p(self.running_loss), int(first), *tail, _lib.stream(self.device)), who)
        self.last_idx = idx
        return loss

    def train(self, ring: PopulationReplayMemory, done: bool, generator: Optional[torch.Generator] = None, minibatch: int = 264,
              min_replay: int = 1000, spec=None):
        """The reference's train for every member at once: 0 below min_replay, else a step on `minibatch` rows per member
        drawn on the device (one torch.randint of [P, B]), then the target counter (host side) and the sync."""
        if len(ring) < min_replay:
            return 0
        idx = torch.randint(0, len(ring), (self.n_members, minibatch), device=self.device, generator=generator)
        loss = self.step(ring, idx, spec)
        self._count_target(done)
        return loss


class PopulationLinearTrainer(_PopulationTrainer):
    """LinearTrainer's tensors with a leading [P], trained by antsrl_pop_lintrain_step: one launch, one workgroup per
    member.  w1 [P, 32, F + 2], b1 [P, 32] (frozen), heads [P, 198], target_l3 [P, 99], `_adam` [P, 2, 198], grads
    [P, 198]; member p's weights are initialised as LinearTrainer(seed=seed_p)'s.  Per member: discount and learning rate.
    Common: Adam's betas, eps and step count, update_target_every and the target counter.  `running_loss` (float64 [P])
    is main.py:106-109's running loss per member, kept by the training launch itself from the first training step on."""

    def __init__(self, geometry: _Geometry, device, seeds, discount, lr, betas=(0.9, 0.999), eps: float = 1e-8,
                 update_target_every: int = 1):
        super().__init__(geometry, device, seeds, discount, lr, betas, eps, update_target_every)
        P, F = self.n_members, self.n_features
        sds = [linear_init(dict(layer1=(32, F + 2), layer2=(3, 32), layer3=(3, 32)), s) for s in self.seeds]
        stack = lambda f: torch.stack([f(sd) for sd in sds]).to(self.device).contiguous()  # noqa: E731
        self.w1, self.b1 = stack(lambda sd: sd["layer1.weight"]), stack(lambda sd: sd["layer1.bias"])
        self.heads = stack(lambda sd: torch.cat([sd["layer2.weight"].reshape(-1), sd["layer2.bias"],
                                                 sd["layer3.weight"].reshape(-1), sd["layer3.bias"]]))
        self.target_l3 = self.heads[:, 99:198].clone()
        self._adam = torch.zeros((P, 2, 198), dtype=torch.float32, device=self.device)
        self.grads = torch.zeros((P, 198), dtype=torch.float32, device=self.device)

    # ---- weights ------------------------------------------------------------------------------------------------------
    def _model_views(self, p: int) -> dict:
        return linear_model_views(self.w1[p], self.b1[p], self.heads[p])

    def state_dict(self, p: int) -> dict:
        """Member p's six tensors (copies) under CollectModel's names, in its order: what the reference loads."""
        return _clones(self._model_views(p))

    def target_state_dict(self, p: int) -> dict:
        return linear_target_state_dict(self.state_dict(p), self.target_l3[p])

    def _load(self, sd, p: Optional[int], names) -> None:
        sd = collect_names(sd)
        for q in range(self.n_members)[_rows(p)]:
            copy_named(sd, self._model_views(q), names)

    def load_state_dict(self, sd, p: Optional[int] = None) -> None:
        """LinearTrainer.load_state_dict for member p (None: every member): model AND target; Adam's state is kept."""
        self._load(sd, p, LINEAR_NAMES)
        rows = _rows(p)
        self.target_l3[rows].copy_(self.heads[rows, 99:198])

    def load_explore_state_dict(self, sd, p: Optional[int] = None) -> None:
        """LinearTrainer.load_explore_state_dict for member p (None: every member): layer1 and layer2 from a four-tensor
        ExploreModel state_dict; layer3, its target copy and Adam's state stay."""
        self._load(sd, p, LINEAR_NAMES[:4])

    def load_explore_population(self, explore_trainer) -> None:
        """The hand-over from stage 1 of the curriculum for every member at once: member p's layer1 and layer2 from
        member p's MODEL block of a PopulationExploreTrainer (w1 | b1 | w2 | b2 in one flat block; heads[:99] is w2 | b2),
        three device copies of [P, ...].  layer3, its target copy and Adam's state stay, as load_explore_state_dict
        leaves them."""
        P, n1 = self.n_members, 32 * (self.n_features + 2)
        _same_population(self, explore_trainer, "explore")
        m = explore_trainer.model.to(self.device)
        self.w1.view(P, n1).copy_(m[:, :n1])
        self.b1.copy_(m[:, n1:n1 + 32])
        self.heads[:, :99].copy_(m[:, n1 + 32:n1 + 131])

    def adam_state(self, p: int) -> dict:
        return linear_adam_state(self.step_count, self._adam[p])

    def sync_target(self) -> None:
        """target := model for every member: one copy of [P, 99]."""
        self.target_l3.copy_(self.heads[:, 99:198])
        self.syncs += 1

    def _entry(self) -> tuple:
        """One launch."""
        return (self._lib.antsrl_pop_lintrain_step, "pop_lintrain_step",
                (_p(self.w1), _p(self.b1), _p(self.heads), _p(self.target_l3), _p(self._adam)))

    def _workspace_bytes(self, B: int) -> None:
        """The one launch keeps a member's minibatch in its workgroup: no workspace."""
        return None


class _PopulationFlatTrainer(_PopulationTrainer):
    """What the explore, the joint and the rework population trainer share, train._FlatTrainer's counterpart for a population: a
    member's net is ONE flat block described by `_offs` (name -> (offset, shape)); `model`, `_adam[0]`, `_adam[1]` and
    grads are [P, trained_floats]; the entries are antsrl_pop_<entry>_sizes / _step and take (model, the target, Adam's m,
    Adam's v) in front of the ring's arrays.  A subclass names its `entry` and the tensor that is its `target_name`, lists
    its layers (`_alloc_flat`), allocates its target and writes sync_target and its loads."""

    entry = None  # "exptrain", "jointtrain", "reworktrain" (whose entries take the net's shape in front: it overrides _sizes and _entry)
    target_name = None  # the attribute the step entry takes behind `model`

    def _alloc_flat(self, names: Sequence[str], layers: dict) -> None:
        """The table of a block whose tensors are `names` in order, a weight and a bias per layer of `layers` (name ->
        (out, in), a block's order); `model`, member p's drawn as the single trainer's by linear_init(layers, seed_p);
        Adam's moments and the gradients, zeroed."""
        P = self.n_members
        self._offs, off = {}, 0
        for k, shp in zip(names, (s for out_f, in_f in layers.values() for s in ((out_f, in_f), (out_f,)))):
            self._offs[k] = (off, shp)
            off += math.prod(shp)
        self._step_name = "pop_%s_step" % self.entry
        self._step = getattr(self._lib, "antsrl_" + self._step_name)
        self.trained_floats = self._sizes(1)[0]
        assert self.trained_floats == off
        self.model = torch.stack([torch.cat([t.reshape(-1) for t in linear_init(layers, s).values()])
                                  for s in self.seeds]).to(self.device).contiguous()
        self._adam = torch.zeros((2, P, self.trained_floats), dtype=torch.float32, device=self.device)
        self.grads = torch.zeros((P, self.trained_floats), dtype=torch.float32, device=self.device)

    def _sizes(self, B: int) -> tuple:
        """antsrl_pop_<entry>_sizes -> (trained_floats, a member's workspace stride, the workspace's bytes, launches)."""
        name = "pop_%s_sizes" % self.entry
        tf, stride, ws, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int32()
        _lib.check(getattr(self._lib, "antsrl_" + name)(self.n_features, B, self.n_members, C.byref(tf), C.byref(stride),
                                                        C.byref(ws), C.byref(n)), name)
        return tf.value, stride.value, ws.value, n.value

    def _workspace_bytes(self, B: int) -> int:
        return self._sizes(B)[2]

    def _views(self, flat) -> dict:
        """The tensors of one member's flat block (views) under the reference's names, in its order."""
        return {k: flat[o: o + math.prod(shp)].view(shp) for k, (o, shp) in self._offs.items()}

    def state_dict(self, p: int) -> dict:
        """Member p's tensors (copies) under the reference's names, in its order: what the single agent saves and loads."""
        return _clones(self._views(self.model[p]))

    def adam_state(self, p: int) -> dict:
        return dict(step=self.step_count, exp_avg=_clones(self._views(self._adam[0, p])),
                    exp_avg_sq=_clones(self._views(self._adam[1, p])))

    def _entry(self) -> tuple:
        """Two launches."""
        return (self._step, self._step_name,
                (_p(self.model), _p(getattr(self, self.target_name)), _p(self._adam[0]), _p(self._adam[1])))


class PopulationExploreTrainer(_PopulationFlatTrainer):
    """ExploreTrainer's tensors with a leading [P], trained by antsrl_pop_exptrain_step: two launches whatever P is.
    model, target, `_adam[0]`, `_adam[1]` and grads are [P, trained_floats] (a member's flat block is ExploreTrainer's:
    layer1.weight, layer1.bias, layer2.weight, layer2.bias); member p's weights are initialised as
    ExploreTrainer(seed=seed_p)'s, its target a copy.  The acting net of a member is its TARGET block.  Per member:
    discount and learning rate.  Common: Adam's betas, eps and step count, update_target_every and the target counter.
    `running_loss` (float64 [P]) is kept by the step's second launch from the first training step on."""

    entry, target_name = "exptrain", "target"

    def __init__(self, geometry: _Geometry, device, seeds, discount, lr, betas=(0.9, 0.999), eps: float = 1e-8,
                 update_target_every: int = 1):
        super().__init__(geometry, device, seeds, discount, lr, betas, eps, update_target_every)
        IN = self.n_features + 2
        self._alloc_flat(EXPLORE_NAMES, dict(layer1=(32, IN), layer2=(3, 32)))
        assert self.trained_floats == 32 * IN + 131
        self.target = self.model.clone()

    def target_state_dict(self, p: int) -> dict:
        return _clones(self._views(self.target[p]))

    def load_state_dict(self, sd, p: Optional[int] = None) -> None:
        """ExploreTrainer.load_state_dict for member p (None: every member): model AND target; Adam's state is kept."""
        sd, rows = explore_names(sd), _rows(p)
        for q in range(self.n_members)[rows]:
            copy_named(sd, self._views(self.model[q]))
        self.target[rows].copy_(self.model[rows])

    def sync_target(self) -> None:
        """target := model for every member: one copy of [P, trained_floats]."""
        self.target.copy_(self.model)
        self.syncs += 1

    def train(self, ring: PopulationReplayMemory, done: bool, generator: Optional[torch.Generator] = None, minibatch: int = 256,
              min_replay: int = 1000, spec=None):
        """_PopulationTrainer.train with ExploreAgent's minibatch of 256 as the default."""
        return super().train(ring, done, generator, minibatch, min_replay, spec)


class PopulationJointTrainer(_PopulationFlatTrainer):
    """JointTrainer's tensors with a leading [P], trained by antsrl_pop_jointtrain_step: two launches whatever P is.
    model, `_adam[0]`, `_adam[1]` and grads are [P, trained_floats] (a member's flat block is JointTrainer's: the six
    tensors in CollectModel.state_dict()'s order), target_l3 is [P, 99]; member p's weights are initialised as
    JointTrainer(seed=seed_p)'s, its target layer3 a copy.  The acting net of a member is layer1 and layer2 of its LIVE
    block and its target layer3.  Per member: discount and learning rate.  Common: Adam's betas, eps and step count,
    update_target_every and the target counter.  `running_loss` (float64 [P]) is kept by the step's second launch from
    the first training step on."""

    entry, target_name = "jointtrain", "target_l3"

    def __init__(self, geometry: _Geometry, device, seeds, discount, lr, betas=(0.9, 0.999), eps: float = 1e-8,
                 update_target_every: int = 1):
        super().__init__(geometry, device, seeds, discount, lr, betas, eps, update_target_every)
        IN = self.n_features + 2
        self._alloc_flat(LINEAR_NAMES, dict(layer1=(32, IN), layer2=(3, 32), layer3=(3, 32)))
        off = self.trained_floats
        assert off == 32 * IN + 230
        self._l3 = slice(off - 99, off)  # layer3 in a block: the 99 floats the target copies
        self.target_l3 = self.model[:, self._l3].clone()

    def target_state_dict(self, p: int) -> dict:
        return linear_target_state_dict(self.state_dict(p), self.target_l3[p])

    def _load(self, sd, p: Optional[int], names) -> None:
        sd = collect_names(sd)
        for q in range(self.n_members)[_rows(p)]:
            copy_named(sd, self._views(self.model[q]), names)

    def load_state_dict(self, sd, p: Optional[int] = None) -> None:
        """JointTrainer.load_state_dict for member p (None: every member): model AND target; Adam's state is kept."""
        self._load(sd, p, LINEAR_NAMES)
        rows = _rows(p)
        self.target_l3[rows].copy_(self.model[rows, self._l3])

    def load_explore_state_dict(self, sd, p: Optional[int] = None) -> None:
        """JointTrainer.load_explore_state_dict for member p (None: every member): layer1 and layer2 from a four-tensor
        ExploreModel state_dict; layer3, its target copy and Adam's state stay."""
        self._load(sd, p, LINEAR_NAMES[:4])

    def load_explore_population(self, explore_trainer) -> None:
        """PopulationLinearTrainer.load_explore_population for this net: a member's explore block (w1 | b1 | w2 | b2) is
        the front of its joint block, one device copy of [P, 32 (F + 2) + 131]."""
        _same_population(self, explore_trainer, "explore")
        n = explore_trainer.trained_floats
        self.model[:, :n].copy_(explore_trainer.model.to(self.device))

    def load_collect_population(self, linear_trainer) -> None:
        """The hand-over from stage 2 of the curriculum for every member at once: member p's w1, b1 and heads from a
        PopulationLinearTrainer into its block (w1 | b1 | heads), three device copies of [P, ...]; target_l3 becomes the
        block's layer3; Adam's state stays zero as it is.  For every p it is load_state_dict(linear_trainer.state_dict(p), p)."""
        P, n1 = self.n_members, 32 * (self.n_features + 2)
        _same_population(self, linear_trainer, "collect")
        self.model[:, :n1].copy_(linear_trainer.w1.to(self.device).view(P, n1))
        self.model[:, n1:n1 + 32].copy_(linear_trainer.b1.to(self.device))
        self.model[:, n1 + 32:].copy_(linear_trainer.heads.to(self.device))
        self.target_l3.copy_(self.model[:, self._l3])

    def sync_target(self) -> None:
        """target := model for every member: one copy of [P, 99]."""
        self.target_l3.copy_(self.model[:, self._l3])
        self.syncs += 1


class PopulationMemoryTrainer(_MemoryBlocks, _PopulationTrainer):
    """MemoryTrainer's state buffers with a leading [P], trained by antsrl_pop_memtrain_step: 17 launches whatever P is
    (16 of the gradient stage, 1 of Adam and the repack).  `_model` and `_target` are uint8 [P, state_stride], a member's
    block MemoryTrainer's buffer (masters, Adam's m and v, the bf16 packs); grads is [P, trained_floats].  Member p is
    initialised as MemoryTrainer(seed=seed_p) is, its target a copy.  Per member: discount and learning rate.  Common:
    the net's shape, Adam's betas, eps and step count, update_target_every and the target counter.  `running_loss`
    (float64 [P]) is kept by the finalize launch from the first training step on.  The ring of a step is a
    PopulationReplayMemory(..., agent_states_space=(2 + mem_size,)).

    `packed` (uint8 [P, pack_stride]) holds every member's ACTING net, its TARGET net as antsrl_memnet_pack_ex packs it
    in bf16 (MemoryTrainer's `policy.packed` per member): what antsrl_pop_policy_memory acts with.  `_repack_policy`
    packs it again, P launches, at construction, sync_target and load_state_dict; the step does not touch it."""

    def __init__(self, geometry: _Geometry, device, seeds, discount, lr, betas=(0.9, 0.999), eps: float = 1e-8,
                 update_target_every: int = 1, *, power: int = 5, mem_size: int = 20, n_rot: int = 3, n_ph: int = 3):
        super().__init__(geometry, device, seeds, discount, lr, betas, eps, update_target_every)
        P, F = self.n_members, self.n_features
        self._init_blocks(memnet_shape(F, power, mem_size, n_rot, n_ph), F, power, mem_size, n_rot, n_ph)
        self.state_stride, tf = self._sizes(1)[:2]
        assert self.state_stride == self.state_bytes and tf == self.trained_floats and self.state_stride % 256 == 0
        self._model = torch.empty((P, self.state_stride), dtype=torch.uint8, device=self.device)
        self._target = torch.empty_like(self._model)
        self.grads = torch.zeros((P, self.trained_floats), dtype=torch.float32, device=self.device)
        shapes = memnet_param_shapes(F, power, mem_size, n_rot, n_ph)
        for p, seed in enumerate(self.seeds):
            self._init_state(linear_init(shapes, seed), (self._model[p], self._target[p]))
        stride, total = C.c_size_t(), C.c_size_t()
        _lib.check(self._lib.antsrl_pop_memnet_sizes(C.byref(self.shape), MEMNET_PRECISIONS["bf16"], P, C.byref(stride),
                                                     C.byref(total)), "pop_memnet_sizes")
        self.pack_stride = stride.value
        assert total.value == P * self.pack_stride and self.pack_stride % 256 == 0
        self.packed = torch.zeros((P, self.pack_stride), dtype=torch.uint8, device=self.device)  # (torch blocks are 512-byte aligned)
        self._repack_policy()

    def _repack_policy(self, p: Optional[int] = None) -> None:
        """MemoryTrainer._repack_policy for member p (None: every member): its block of `packed` := its target net,
        antsrl_memnet_pack_ex in bf16 straight from the target's masters."""
        with torch.cuda.device(self.device):
            for q in range(self.n_members)[_rows(p)]:
                ptrs = memnet_param_ptrs(self._views(self._target[q]))
                _lib.check(self._lib.antsrl_memnet_pack_ex(C.byref(self.shape), MEMNET_PRECISIONS["bf16"], ptrs,
                                                           _p(self.packed[q]), _lib.stream(self.device)), "memnet_pack_ex")

    def _sizes(self, B: int) -> tuple:
        """antsrl_pop_memtrain_sizes -> (a member's state stride, trained_floats, a member's workspace stride, the
        workspace's bytes, launches)."""
        ss, tf, stride, ws, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int32()
        _lib.check(self._lib.antsrl_pop_memtrain_sizes(C.byref(self.shape), B, self.n_members, C.byref(ss), C.byref(tf),
                                                       C.byref(stride), C.byref(ws), C.byref(n)), "pop_memtrain_sizes")
        return ss.value, tf.value, stride.value, ws.value, n.value

    # ---- weights ------------------------------------------------------------------------------------------------------
    def state_dict(self, p: int) -> dict:
        """Member p's 26 tensors (copies) under CollectModelMemory's names, in its order: what the reference loads."""
        return _clones(self._views(self._model[p]))

    def target_state_dict(self, p: int) -> dict:
        return _clones(self._views(self._target[p]))

    def load_state_dict(self, sd, p: Optional[int] = None) -> None:
        """MemoryTrainer.load_state_dict for member p (None: every member): model AND target (and the acting pack);
        Adam's state is kept."""
        for q in range(self.n_members)[_rows(p)]:
            keep = self._model[q, self._adam_range()].clone()
            self._init_state(sd, (self._model[q], self._target[q]))
            self._model[q, self._adam_range()] = keep
        self._repack_policy(p)

    def adam_state(self, p: int) -> dict:
        return self._adam_dict(self._model[p], self.step_count)

    def sync_target(self) -> None:
        """target := model for every member (antsrl_memtrain_copy on its block: masters and packs, not Adam's moments),
        and the acting packs with it."""
        with torch.cuda.device(self.device):
            for p in range(self.n_members):
                _lib.check(self._lib.antsrl_memtrain_copy(C.byref(self.shape), _p(self._model[p]), _p(self._target[p]),
                                                          _lib.stream(self.device)), "memtrain_copy")
        self._repack_policy()
        self.syncs += 1

    # ---- the step -----------------------------------------------------------------------------------------------------
    def _workspace_bytes(self, B: int) -> int:
        return self._sizes(B)[3]

    def _entry(self) -> tuple:
        """17 launches; the shape leads the net's pointers."""
        return (self._lib.antsrl_pop_memtrain_step, "pop_memtrain_step", (C.byref(self.shape), _p(self._model), _p(self._target)))


class PopulationReworkTrainer(_PopulationFlatTrainer):
    """ReworkTrainer's tensors with a leading [P], trained by antsrl_pop_reworktrain_step: the single step's four
    launches whatever P is.  model, target, `_adam[0]`, `_adam[1]` and grads are [P, trained_floats] (a member's flat
    block is ReworkTrainer's: CollectModelRework's twenty tensors in its state_dict's order), `collapsed` is
    [P, NQ D + NQ]: member p's TARGET block multiplied out (ReworkPolicy's collapsed buffer), what the population acts
    with and the step takes its TD targets from.  Member p's weights are initialised as ReworkPolicy(seed=seed_p)
    initialises a lone net, its target a copy.  Per member: discount and learning rate.  Common: the net's shape (the
    heads' widths; the reference's hidden widths), Adam's betas, eps and step count, update_target_every and the target
    counter.  `running_loss` (float64 [P]) is kept by the step's third launch from the first training step on.

    sync_target and load_state_dict copy blocks and collapse ONCE for all members (antsrl_pop_rework_collapse); a
    training step changes neither `collapsed` nor `version`, which counts the changes of the acting weights as
    ReworkTrainer's does."""

    entry, target_name = "reworktrain", "collapsed"

    def __init__(self, geometry: _Geometry, device, seeds, discount, lr, betas=(0.9, 0.999), eps: float = 1e-8,
                 update_target_every: int = 1, *, n_rot: int = 3, n_ph: int = 3):
        super().__init__(geometry, device, seeds, discount, lr, betas, eps, update_target_every)
        layers = rework_param_shapes(self.n_features, n_rot, n_ph)
        shp = dict(n_features=self.n_features, agent_dim=2, n_rot=n_rot, n_ph=n_ph,
                   **{k: layers[l][0] for k, l in (("g1", "layer1"), ("g2", "layer2"), ("g3", "layer3"), ("r1", "rotation_layer1"),
                                                   ("r2", "rotation_layer2"), ("r3", "rotation_layer3"), ("p1", "pheromone_layer1"))})
        self.n_rot, self.n_ph = n_rot, n_ph
        self.shape = _lib.AntsReworkShape(*[shp[n] for n, _ in _lib.AntsReworkShape._fields_])
        self._alloc_flat(["%s.%s" % (l, w) for l in REWORK_LAYERS for w in ("weight", "bias")], layers)
        self.collapsed_floats = self._sizes(1)[4]
        assert self.collapsed_floats == (n_rot + n_ph) * (self.n_features + 3)
        self.target = self.model.clone()
        self.collapsed = torch.empty((self.n_members, self.collapsed_floats), dtype=torch.float32, device=self.device)
        self.version = 0
        self._collapse()

    def _sizes(self, B: int) -> tuple:
        """antsrl_pop_reworktrain_sizes -> (trained_floats, a member's workspace stride, the workspace's bytes, launches,
        the floats of a member's collapsed buffer)."""
        tf, cf, stride, ws, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int32()
        _lib.check(self._lib.antsrl_pop_reworktrain_sizes(C.byref(self.shape), B, self.n_members, C.byref(tf), C.byref(cf),
                                                          C.byref(stride), C.byref(ws), C.byref(n)), "pop_reworktrain_sizes")
        return tf.value, stride.value, ws.value, n.value, cf.value

    def _collapse(self) -> None:
        """`collapsed` := every member's target block multiplied out: one launch."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_pop_rework_collapse(C.byref(self.shape), self.n_members, _p(self.target), _p(self.collapsed),
                                                            _lib.stream(self.device)), "pop_rework_collapse")

    def target_state_dict(self, p: int) -> dict:
        return _clones(self._views(self.target[p]))

    def load_state_dict(self, sd, p: Optional[int] = None) -> None:
        """ReworkTrainer.load_state_dict for member p (None: every member): model AND target, then the collapse; Adam's
        state is kept.  The widths are the population's: a state_dict of another shape is refused."""
        rows = _rows(p)
        for q in range(self.n_members)[rows]:
            copy_named(sd, self._views(self.model[q]))
        self.target[rows].copy_(self.model[rows])
        self._collapse()
        self.version += 1

    def sync_target(self) -> None:
        """target := model for every member: one copy of [P, trained_floats] and one collapse launch."""
        self.target.copy_(self.model)
        self._collapse()
        self.syncs += 1
        self.version += 1

    def _entry(self) -> tuple:
        """Four launches; the shape leads the net's pointers."""
        return (self._step, self._step_name, (C.byref(self.shape),) + super()._entry()[2])


def _same_population(trainer, other, kind: str) -> None:
    """A hand-over between two population trainers needs as many members and as wide rows: load_explore_population's
    words, with the handing population's kind."""
    if other.n_members != trainer.n_members:
        raise ValueError("the %s population has %d members, this one %d" % (kind, other.n_members, trainer.n_members))
    if other.n_features != trainer.n_features:
        raise ValueError("the %s population's rows have %d features, these %d" % (kind, other.n_features, trainer.n_features))


class _Population(_LoopAgent):
    """What the populations share around their nets: the members' host values, the front of setup, the step's one
    AntsPopSpec, get_action, the ring, train, the fused loop, the per-member files and copy_member.  A subclass names
    its `minibatch` default in its __init__ and its trainer's class (`trainer_cls`), launches its acting net (`_policy`),
    says whether the net has a pheromone head (`pheromones`) and lists the per-member tensors of its trainer
    (`_member_tensors`); one whose net carries a memory has a select of its own (`_select`) and hands more than the
    actions out of get_action (`_acted`)."""

    rotations = 3
    trainer_cls = None

    def __init__(self, members: Sequence[dict], *, record_per_step: Optional[int], replay_size: int, minibatch: int,
                 min_replay: int, update_target_every: int, seed: int):
        self.members = _members(members)
        self.n_members = len(self.members)
        self._epsilon = np.array([m["epsilon"] for m in self.members], dtype=np.float64)
        self.record_per_step, self.replay_size, self.minibatch, self.min_replay = record_per_step, replay_size, minibatch, min_replay
        self.update_target_every, self.seed = update_target_every, seed
        self.trainer = self.replay_memory = self.generator = None
        self.step_counter = 0
        self._step_spec = None  # rollout_step's: one AntsPopSpec for the step's entries
        self._lib = _lib.load()

    @property
    def epsilon(self) -> np.ndarray:
        """float64 [P]; settable with an array or one number for every member."""
        return self._epsilon

    @epsilon.setter
    def epsilon(self, v) -> None:
        self._epsilon = np.broadcast_to(np.asarray(v, dtype=np.float64), (self.n_members,)).copy()

    def _setup(self, api_or_env, trainer_kw: Optional[dict] = None, agent_states_space: Sequence[int] = (2,)):
        """The front of setup: the geometry, the trainer (a `trainer_cls`; trainer_kw: what its net takes by name beyond the common
        arguments), the ring (agent_states_space: the width of its agent_states rows), the action buffers, the generator
        and the counters."""
        env = _backend(api_or_env)
        cfg = env.cfg
        self.device = env.device
        self.observation_space = tuple(env.obs.shape[-3:])
        self.n_features = int(np.prod(self.observation_space))
        self.g = _Geometry(self.n_members, cfg.n_envs, cfg.n_ants, cfg.env_id_base, self.n_features, env.obs.dtype)
        if self.record_per_step is not None and not 1 <= self.record_per_step <= self.g.Mm:
            raise ValueError("record_per_step = %d is not in [1, %d], a member's ants" % (self.record_per_step, self.g.Mm))
        self.seeds = [m["seed"] for m in self.members]
        self.trainer = self.trainer_cls(self.g, self.device, self.seeds, [m["discount"] for m in self.members],
                                        [m["learning_rate"] for m in self.members], update_target_every=self.update_target_every,
                                        **(trainer_kw or {}))
        self.replay_memory = PopulationReplayMemory(self.n_members, self.replay_size, self.observation_space, device=self.device,
                                                    agent_states_space=agent_states_space)
        M = cfg.n_envs * cfg.n_ants
        self._rot = torch.zeros((M,), dtype=torch.int8, device=self.device)
        self._ph = torch.zeros((M,), dtype=torch.int8, device=self.device)
        self._explored = torch.zeros((cfg.n_envs,), dtype=torch.uint8, device=self.device)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(self.seed)
        self.step_counter = self._action_step = 0
        return env

    def _spec(self, spec=None):
        """This step's AntsPopSpec: the caller's, else rollout_step's, else the one of the values as they are now (the
        kept one while no epsilon, learning rate or discount has changed: the lookup walks 4 P host values)."""
        if spec is None:
            spec = self._step_spec
        tr = self.trainer
        return self.g.spec(self.seeds, self._epsilon, tr.lr, tr.discount) if spec is None else spec

    def _policy(self, spec, obs, agent_state, st) -> None:
        """The acting net of every member into `_rot` (and `_ph`, with a pheromone head)."""
        raise NotImplementedError

    def _select(self, spec, step: int, st) -> None:
        """antsrl_pop_select on `_rot` / `_ph`: the environments that explore at (a member's seed, step) take uniform
        actions."""
        _lib.check(self._lib.antsrl_pop_select(C.byref(spec), step, _p(self._rot), _p(self._ph), _p(self._explored), st), "pop_select")

    def _act(self, spec, obs, agent_state, training: bool, step: int, st) -> None:
        """The step's acting launches: `_policy`, and with `training` `_select` behind it.  (The rework agent fuses the
        two into one launch.)"""
        self._policy(spec, obs, agent_state, st)
        if training:
            self._select(spec, step, st)

    def _acted(self, lead) -> tuple:
        """What get_action returns once the step's launches are enqueued: the actions, shaped like the batch."""
        return self._rot.view(lead), (self._ph.view(lead) if self.pheromones else None)

    def get_action(self, obs, agent_state, training: bool, env=None, spec=None):
        """-> (rotation int8, pheromone int8 or None for a net without that head[, the new memory of a net that carries
        one]), device tensors shaped like the batch: every member's acting net on its own rows (`_policy`); with
        `training`, `_select` then replaces the actions of the environments that explore this step, each member with its
        own seed and epsilon."""
        assert obs.is_contiguous() and agent_state.is_contiguous() and obs.numel() == self._rot.numel() * self.n_features, \
            "a population reads the dense observation rows of its whole batch"
        assert (obs.dtype == torch.bfloat16) == (self.g.obs_format == 1), "the observation's dtype changed since setup"
        step, spec = self.step_counter, self._spec(spec)
        lead = obs.shape[:-3]
        with torch.cuda.device(self.device):
            st = _lib.stream(self.device)
            self._act(spec, obs, agent_state, training, step, st)
        self._action_step = step
        self.step_counter += 1
        return self._acted(lead)

    def train(self, done: bool, step: int = 0, spec=None):
        """0 below min_replay, else the losses of one step of every member, float32 [P] on the device."""
        return self.trainer.train(self.replay_memory, bool(done), generator=self.generator, minibatch=self.minibatch,
                                  min_replay=self.min_replay, spec=self._spec(spec))

    def _record_kw(self) -> dict:
        k = self.g.Mm if self.record_per_step is None else self.record_per_step
        return dict(spec=self._spec(), step=self._action_step, k=k)

    def rollout_step(self, env, training: bool = True):
        """_LoopAgent's step for every member: act, select, record_pre, env.step_update, record_post, train, on ONE lookup
        of the AntsPopSpec.  Returns the losses (float32 [P] on the device; 0 below min_replay or when not training).  No
        host synchronisation."""
        self._step_spec = self._spec()
        try:
            return super().rollout_step(env, training)
        finally:
            self._step_spec = None

    # ---- models -------------------------------------------------------------------------------------------------------
    def save_model(self, p: int, file_name: str) -> None:
        """torch.save of member p's state_dict under the reference's names (on the CPU)."""
        torch.save({k: v.cpu() for k, v in self.trainer.state_dict(p).items()}, file_name)

    def load_model(self, file_name: str, p: Optional[int] = None) -> None:
        """Model and target net of member p (None: of every member) from a state_dict file of the reference's."""
        self.trainer.load_state_dict(torch.load(file_name, map_location="cpu"), p)

    def _member_tensors(self) -> tuple:
        """(tensor, the dimension that counts the members) for every per-member tensor of the trainer."""
        raise NotImplementedError

    def _member_arrays(self, ring: bool) -> list:
        """[(address, bytes of a member's row)] of every per-member array, members outermost: what `_member_tensors`
        lists (a tensor whose member dimension is 1, `_adam` [2][P][...], as one array per leading index) and, with
        `ring`, the ring's seven arrays."""
        out = []
        for t, dim in self._member_tensors() + (tuple((a, 0) for a in ring_arrays(self.replay_memory)) if ring else ()):
            assert t.is_contiguous() and dim in (0, 1) and t.shape[dim] == self.n_members, (tuple(t.shape), dim)
            for part in ((t,) if dim == 0 else t.unbind(0)):
                out.append((part.data_ptr(), part[0].numel() * part.element_size()))
        return out

    def exploit(self, src: Sequence[int], dst: Sequence[int], ring: bool = True) -> None:
        """The exploit step of population-based training: for every pair i, member src[i]'s weights, target, Adam
        moments, what else `_member_tensors` lists and, with `ring`, ring slab over member dst[i]'s, all pairs and all
        arrays in ONE launch (antsrl_pop_exploit).  A src may repeat; a dst may neither repeat nor be a src.  The
        hyper-parameters, seeds and epsilons stay where they are.  No host synchronisation."""
        src, dst = [int(v) for v in src], [int(v) for v in dst]
        assert len(src) == len(dst), "one dst per src (%d, %d)" % (len(src), len(dst))
        if not src:
            return
        arrays = self._member_arrays(ring)
        n = len(arrays)
        base = (C.c_void_p * n)(*[a for a, _ in arrays])
        row_bytes = (C.c_uint64 * n)(*[b for _, b in arrays])
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_pop_exploit(n, base, row_bytes, self.n_members, len(src), (C.c_int32 * len(src))(*src),
                                                    (C.c_int32 * len(dst))(*dst), _lib.stream(self.device)), "pop_exploit")

    def copy_member(self, src: int, dst: int, ring: bool = True) -> None:
        """Member src's weights, target, Adam moments and, with `ring`, ring slab over member dst's: `exploit` of one
        pair; with env.fork the exploit step of population-based training.  The hyper-parameters stay dst's own."""
        P = self.n_members
        assert 0 <= src < P and 0 <= dst < P, (src, dst)
        if src == dst:
            return
        self.exploit([src], [dst], ring)


class PopulationAgent(_Population):
    """P CollectAgents in lockstep (the module docstring).  members: one dict(epsilon=, discount=, learning_rate=, seed=)
    per member (CollectAgent's defaults where a key is missing).  Common to all members: record_per_step (K rows per
    member and step; None: all Em * n_ants), replay_size, minibatch (B <= 512), min_replay, update_target_every; `seed`
    seeds the generator of the minibatch indices.  The acting kernel is always the standalone one."""

    name = "collect_agent_population"
    pheromones = 3
    trainer_cls = PopulationLinearTrainer

    def __init__(self, members: Sequence[dict], *, record_per_step: Optional[int] = None, replay_size: int = 50000,
                 minibatch: int = 264, min_replay: int = 1000, update_target_every: int = 1, seed: int = 0):
        super().__init__(members, record_per_step=record_per_step, replay_size=replay_size, minibatch=minibatch,
                         min_replay=min_replay, update_target_every=update_target_every, seed=seed)

    def setup(self, api_or_env, trained_model: Optional[str] = None, explore_model: Optional[str] = None,
              explore_population=None) -> None:
        """CollectAgent.setup for every member; trained_model / explore_model go to every member.  explore_population: a
        PopulationExploreAgent of as many members, the curriculum's first stage: member p's layer1 and layer2 come from
        its member p's model, device to device (the trainer's load_explore_population); applied last."""
        self._setup(api_or_env)
        if trained_model is not None:
            self.load_model(trained_model)
        if explore_model is not None:
            self.trainer.load_explore_state_dict(torch.load(explore_model, map_location="cpu"))
        if explore_population is not None:
            self.trainer.load_explore_population(explore_population.trainer)

    def _policy(self, spec, obs, agent_state, st) -> None:
        tr = self.trainer
        _lib.check(self._lib.antsrl_pop_policy(C.byref(spec), _p(obs), _p(agent_state), _p(tr.w1), _p(tr.b1), _p(tr.heads),
                                               _p(tr.target_l3), _p(self._rot), _p(self._ph), st), "pop_policy")

    def _member_tensors(self) -> tuple:
        """The frozen layer1 included."""
        tr = self.trainer
        return tuple((t, 0) for t in (tr.w1, tr.b1, tr.heads, tr.target_l3, tr._adam))


class PopulationJointAgent(PopulationAgent):
    """P CollectAgents with the freeze of layer1 lifted (CollectAgent(train_layer1=True)) in lockstep: the third stage
    of the curriculum for every member of a sweep (the module docstring).  members and the common arguments are
    PopulationAgent's (minibatch 264; B <= 512).  The acting net of a member is layer1 and layer2 of its LIVE block and
    its target layer3: every training step moves it.  Take its members' nets from a PopulationAgent with
    setup(env, collect_population=that)."""

    name = "joint_agent_population"
    trainer_cls = PopulationJointTrainer

    def setup(self, api_or_env, trained_model: Optional[str] = None, explore_model: Optional[str] = None,
              explore_population=None, collect_population=None) -> None:
        """PopulationAgent.setup with all six tensors trained.  collect_population: a PopulationAgent of as many members,
        the curriculum's second stage: member p's six tensors come from its member p, device to device
        (PopulationJointTrainer.load_collect_population); applied last."""
        super().setup(api_or_env, trained_model, explore_model, explore_population)
        if collect_population is not None:
            self.trainer.load_collect_population(collect_population.trainer)

    def _policy(self, spec, obs, agent_state, st) -> None:
        tr = self.trainer
        _lib.check(self._lib.antsrl_pop_joint_policy(C.byref(spec), _p(obs), _p(agent_state), _p(tr.model), _p(tr.target_l3),
                                                     _p(self._rot), _p(self._ph), st), "pop_joint_policy")

    def _member_tensors(self) -> tuple:
        tr = self.trainer
        return ((tr.model, 0), (tr.target_l3, 0), (tr._adam, 1))


class PopulationExploreAgent(_Population):
    """P ExploreAgents in lockstep: the first stage of the curriculum for every member of a sweep (the module
    docstring).  Rotation only: get_action returns (rotation, None), the environment is stepped without a pheromone
    action and the ring stores (rotation + 1, 1).  members and the common arguments are PopulationAgent's (ExploreAgent's
    minibatch of 256; B <= 512).  The acting net of a member is its TARGET block, which changes at a sync or a load only.
    Hand its members' layer1 and layer2 to a PopulationAgent with PopulationAgent.setup(env, explore_population=this)."""

    name = "explore_agent_population"
    pheromones = 0  # no pheromone head (antsrl_pop_select still draws a pheromone for every exploring ant: nothing reads it)
    trainer_cls = PopulationExploreTrainer

    def __init__(self, members: Sequence[dict], *, record_per_step: Optional[int] = None, replay_size: int = 50000,
                 minibatch: int = 256, min_replay: int = 1000, update_target_every: int = 1, seed: int = 0):
        super().__init__(members, record_per_step=record_per_step, replay_size=replay_size, minibatch=minibatch,
                         min_replay=min_replay, update_target_every=update_target_every, seed=seed)

    def setup(self, api_or_env, trained_model: Optional[str] = None) -> None:
        """ExploreAgent.setup for every member; trained_model goes to every member."""
        self._setup(api_or_env)
        if trained_model is not None:
            self.load_model(trained_model)

    def _policy(self, spec, obs, agent_state, st) -> None:
        _lib.check(self._lib.antsrl_pop_explore_policy(C.byref(spec), _p(obs), _p(agent_state), _p(self.trainer.target),
                                                       _p(self._rot), st), "pop_explore_policy")

    def _member_tensors(self) -> tuple:
        tr = self.trainer
        return ((tr.model, 0), (tr.target, 0), (tr._adam, 1))


class PopulationMemoryAgent(_Population):
    """P MemoryAgents in lockstep: CollectAgentMemory, the agent main.py trains, for every member of a sweep (the module
    docstring).  members: PopulationAgent's dicts (MemoryAgent's defaults where a key is missing).  Common
    to all members: the net's shape (mem_size, power), `state_memory` ("reference": agent_states rows hold the
    post-action memory, as the reference stores it; "carried": the pre-action memory; antsrl_amd/agent.py says why
    there are two), record_per_step, replay_size, minibatch (the reference's 264), min_replay, update_target_every;
    `seed` seeds the generator of the minibatch indices.

    The acting net of a member is its TARGET net, packed in bf16 (PopulationMemoryTrainer.packed), so it changes at a
    sync or a load only.  get_action returns (rotation, pheromone, the new memory [M, mem_size]): one launch of every
    member's forward (antsrl_pop_policy_memory), with `training` one of antsrl_pop_memory_select (uniform actions and the
    old memory back for the ants of a member's exploring environments), then the two memory halves swap, as
    MemoryAgent's do.  rollout_step is _Population's: one AntsPopSpec per step and no host read.

    Not here: skip_explored (the explore plan and the tile-list forward) and the fp32 acting precision."""

    name = "collect_agent_memory_population"
    pheromones = 3
    trainer_cls = PopulationMemoryTrainer

    def __init__(self, members: Sequence[dict], *, mem_size: int = 20, power: int = 5, state_memory: str = "reference",
                 record_per_step: Optional[int] = None, replay_size: int = 50000, minibatch: int = 264,
                 min_replay: int = 1000, update_target_every: int = 1, seed: int = 0):
        assert state_memory in ("reference", "carried"), "state_memory must be 'reference' or 'carried', not %r" % (state_memory,)
        super().__init__(members, record_per_step=record_per_step, replay_size=replay_size, minibatch=minibatch,
                         min_replay=min_replay, update_target_every=update_target_every, seed=seed)
        self.mem_size, self.power, self.state_memory = mem_size, power, state_memory

    def setup(self, api_or_env, trained_model: Optional[str] = None) -> None:
        """MemoryAgent.setup for every member; trained_model goes to every member."""
        self._setup(api_or_env, dict(power=self.power, mem_size=self.mem_size, n_rot=self.rotations, n_ph=self.pheromones),
                    agent_states_space=(2 + self.mem_size,))
        M = self._rot.numel()
        self._mem = [torch.zeros((M, self.mem_size), dtype=torch.float32, device=self.device) for _ in range(2)]
        self._cur = 0  # self._mem[self._cur] is previous_memory (collect_agent_memory.py:111), every member's rows
        self._memory_before = self._mem[1]
        self._halves = None  # (old, new) of the step get_action is in
        if trained_model is not None:
            self.load_model(trained_model)

    @property
    def previous_memory(self) -> torch.Tensor:
        return self._mem[self._cur]

    def _policy(self, spec, obs, agent_state, st) -> None:
        """Every member's target net on its own rows, the new memory into the other half."""
        tr = self.trainer
        old, new = self._halves = self._mem[self._cur], self._mem[1 - self._cur]
        _lib.check(self._lib.antsrl_pop_policy_memory(C.byref(spec), C.byref(tr.shape), MEMNET_PRECISIONS["bf16"], _p(tr.packed),
                                                      _p(obs), _p(agent_state), _p(old), _p(new), _p(self._rot), _p(self._ph),
                                                      None, st), "pop_policy_memory")

    def _select(self, spec, step: int, st) -> None:
        """antsrl_pop_memory_select: _Population._select, and the ants of the exploring environments get their old memory
        back."""
        old, new = self._halves
        _lib.check(self._lib.antsrl_pop_memory_select(C.byref(spec), C.byref(self.trainer.shape), step, _p(self._rot),
                                                      _p(self._ph), _p(old), _p(new), _p(self._explored), st), "pop_memory_select")

    def _acted(self, lead) -> tuple:
        """(rotation int8, pheromone int8, the new memory float32 [M, mem_size]); the two halves swap, as MemoryAgent's do."""
        self._memory_before, new = self._halves
        self._cur = 1 - self._cur
        return self._rot.view(lead), self._ph.view(lead), new

    def _state_memory(self) -> torch.Tensor:
        """The memory that goes into agent_states (MemoryAgent._state_memory)."""
        return self.previous_memory if self.state_memory == "reference" else self._memory_before

    def _record_kw(self) -> dict:
        return dict(super()._record_kw(), shape=self.trainer.shape)

    def _member_tensors(self) -> tuple:
        """A state block holds the weights AND Adam's moments; the acting pack goes with the target; and a member's rows
        of BOTH memory halves ([P Mm][mem], seen as [P][Mm][mem]).  env.fork copies src's ants into dst's environments; a
        fork without their memory would hand dst's memory, which belongs to the ants that were there before, to src's
        ants.  So copy_member and exploit go with the fork, between two steps."""
        tr = self.trainer
        halves = tuple((m.view(self.n_members, self.g.Mm, self.mem_size), 0) for m in self._mem)
        return ((tr._model, 0), (tr._target, 0), (tr.packed, 0)) + halves


class PopulationReworkAgent(_Population):
    """P ReworkAgents in lockstep: CollectAgentRework, the agent main.py imports first, for every member of a sweep (the
    module docstring).  members: PopulationAgent's dicts (ReworkAgent's defaults where a key is missing).
    Common to all members: the heads' widths (`rotations`, `pheromones`, 1 .. 8 each), `fused_select`, record_per_step,
    replay_size, minibatch (the reference's 264; up to 65536), min_replay, update_target_every; `seed` seeds the
    generator of the minibatch indices.

    The acting net of a member is its TARGET block multiplied out (PopulationReworkTrainer.collapsed), so it changes at
    a sync or a load only.  `fused_select` (on by default): with `training`, act and select are ONE launch for all
    members whatever their epsilons (antsrl_pop_policy_rework_select): a member's pass whose rows all explore is not
    evaluated, a member with epsilon 0 is evaluated on every row.  Off, it is the net on the whole batch
    (antsrl_pop_policy_rework) and antsrl_pop_select behind it.  Both give the same actions, rings, weights and losses
    bit for bit, as ReworkAgent's two forms do.

    The ring and its record halves are the linear population's: they store rotation + 1, so `rotations` is 2 or 3 (a
    wider rotation head acts and trains through the entries, but not through this loop); antsrl_pop_select draws among
    three rotations and three pheromones, so fused_select=False needs both heads three wide."""

    name = "collect_agent_rework_population"
    pheromones = True
    trainer_cls = PopulationReworkTrainer

    def __init__(self, members: Sequence[dict], *, rotations: int = 3, pheromones: int = 3, fused_select: bool = True,
                 record_per_step: Optional[int] = None, replay_size: int = 50000, minibatch: int = 264, min_replay: int = 1000,
                 update_target_every: int = 1, seed: int = 0):
        assert 1 <= rotations <= 8 and 1 <= pheromones <= 8, \
            "the net's heads are 1 to 8 wide (antsrl_pop_policy_rework), not %r and %r" % (rotations, pheromones)
        assert rotations // 2 == 1, "the population's ring stores rotation + 1: rotations must be 2 or 3, not %r" % (rotations,)
        assert fused_select or (rotations, pheromones) == (3, 3), \
            "antsrl_pop_select draws among three rotations and three pheromones: fused_select=False needs heads (3, 3)"
        super().__init__(members, record_per_step=record_per_step, replay_size=replay_size, minibatch=minibatch,
                         min_replay=min_replay, update_target_every=update_target_every, seed=seed)
        self.rotations, self.pheromones, self.fused_select = rotations, pheromones, fused_select

    def setup(self, api_or_env, trained_model: Optional[str] = None) -> None:
        """ReworkAgent.setup for every member; trained_model goes to every member."""
        self._setup(api_or_env, dict(n_rot=self.rotations, n_ph=self.pheromones))
        if trained_model is not None:
            self.load_model(trained_model)

    def _policy(self, spec, obs, agent_state, st) -> None:
        tr = self.trainer
        _lib.check(self._lib.antsrl_pop_policy_rework(C.byref(spec), C.byref(tr.shape), _p(tr.collapsed), _p(obs), _p(agent_state),
                                                      _p(self._rot), _p(self._ph), None, st), "pop_policy_rework")

    def _act(self, spec, obs, agent_state, training: bool, step: int, st) -> None:
        """With `training` and `fused_select`, act and select in one launch; else _Population's two."""
        if not (training and self.fused_select):
            return super()._act(spec, obs, agent_state, training, step, st)
        tr = self.trainer
        _lib.check(self._lib.antsrl_pop_policy_rework_select(C.byref(spec), C.byref(tr.shape), _p(tr.collapsed), _p(obs),
                                                             _p(agent_state), step, _p(self._rot), _p(self._ph),
                                                             _p(self._explored), None, st), "pop_policy_rework_select")

    def _member_tensors(self) -> tuple:
        """The collapsed buffer travels with the target block it was multiplied out of."""
        tr = self.trainer
        return ((tr.model, 0), (tr.target, 0), (tr.collapsed, 0), (tr._adam, 1))
