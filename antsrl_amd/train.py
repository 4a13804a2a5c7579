"""On-device DQN training of the memory agent net: CollectAgentMemory.train (agents/collect_agent_memory.py:133-176) as
two HIP stages, `antsrl_memtrain_grad` (target and model forwards, TD targets, loss, backward into one flat fp32
gradient buffer) and `antsrl_memtrain_apply` (Adam, then the bf16 operand repack).  See antsrl_memtrain.hip and
DESIGN §7.7 for the precision contract.

Each net lives in one device buffer (include/antsrl.h, antsrl_memtrain_sizes): the fp32 masters of the 26 state_dict
tensors in its order, Adam's m and v for the 18 trained tensors, and the bf16 operand packs.  The memory head
(memory_layer1-3, forget_layer) gets no gradient in the reference (its .grad stays None, so Adam skips it): it is never
changed here either, and has no Adam state.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import ptr as _p
from .replay import ring_arrays
from .policy import MEMNET_LAYERS, MemoryPolicy, memnet_param_ptrs, memnet_param_shapes, memnet_shape_from_state_dict

#: the 9 layers the loss reaches (the first 18 tensors of the state_dict)
TRAINED_LAYERS = MEMNET_LAYERS[:9]


class _TargetCounter:
    """The tail of the reference's train behind a training step, for a trainer with `target_update_counter`,
    `update_target_every` and `sync_target`: the counter moves at an episode's end (`done`, a host bool) and the target
    net follows the model when it reaches update_target_every (collect_agent.py:141-146)."""

    def _count_target(self, done: bool) -> None:
        if done:
            self.target_update_counter += 1
        if self.target_update_counter >= self.update_target_every:
            self.sync_target()
            self.target_update_counter = 0


def copy_named(sd, views: dict, names=None) -> None:
    """sd[k] into views[k] for k in names (None: every view), as float32 on the view's device; the shapes must agree."""
    for k in (views if names is None else names):
        dst = views[k]
        src = torch.as_tensor(sd[k]).to(dst.device, torch.float32)
        assert tuple(src.shape) == tuple(dst.shape), (k, tuple(src.shape), tuple(dst.shape))
        dst.copy_(src)


def _clones(views: dict) -> dict:
    return {k: v.clone() for k, v in views.items()}


class _DqnTrainer(_TargetCounter):
    """What the five trainers share: the hyper-parameters and counters, the checks of a minibatch's arrays and its
    workspace, and train() around step().  A subclass holds its nets, writes grad / apply / step over its own entries
    (_FlatTrainer does, for the four whose ABIs share one argument order), sync_target, and
    `_sizes(B, workspace_bytes, launches)`, its antsrl_*train_sizes call."""

    minibatch = 264  # train()'s default: the reference class's

    def __init__(self, n_features: int, device, ast_width: int, discount: float, lr: float, betas, eps: float,
                 update_target_every: int):
        self.device = torch.device(device)
        assert self.device.type == "cuda", "%s runs on the GPU" % type(self).__name__
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_features, self._ast_width = n_features, ast_width  # floats of an observation, of an agent_states row
        self.discount, self.lr, self.betas, self.eps = float(discount), float(lr), tuple(float(b) for b in betas), float(eps)
        self.update_target_every = int(update_target_every)
        self.target_update_counter = 0
        self.syncs = 0
        self.step_count = 0
        self._work = None
        self._lib = _lib.load()

    def _arrays(self, batch_or_replay):
        r = batch_or_replay
        a = ring_arrays(r) if hasattr(r, "states") else tuple(r)
        n = len(r) if hasattr(r, "states") else a[0].shape[0]
        assert len(a) == 7
        st, ast, act, rw, nst, nast, dn = a
        N = st.shape[0]
        for t, dt in ((st, torch.float32), (ast, torch.float32), (act, torch.int64), (rw, torch.float32),
                      (nst, torch.float32), (nast, torch.float32), (dn, torch.bool)):
            assert t.device == self.device and t.dtype == dt and t.is_contiguous() and t.shape[0] == N, (t.shape, t.dtype)
        assert st[0].numel() == self.n_features and nst[0].numel() == self.n_features
        assert ast.shape[1:] == (self._ast_width,) and nast.shape[1:] == (self._ast_width,), \
            "agent_states rows are %d floats" % self._ast_width
        assert act.shape[1:] == (2,) and rw.dim() == 1 and dn.dim() == 1
        return a, n, N

    def _batch(self, batch_or_replay, idx):
        """The seven arrays, their rows N and the minibatch's B, with the workspace grown to what B rows need."""
        a, n, N = self._arrays(batch_or_replay)
        if idx is not None:
            assert idx.device == self.device and idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_contiguous()
            B = idx.numel()
        else:
            B = n
        assert B >= 1
        ws = C.c_size_t()
        self._sizes(B, C.byref(ws), None)
        if self._work is None or self._work.numel() < ws.value:
            self._work = torch.empty((ws.value,), dtype=torch.uint8, device=self.device)
        return a, N, B

    def launches(self, B: int) -> int:
        """Kernel launches of one step on B rows (antsrl_lintrain_sizes: 1 up to 512 rows, else 2; antsrl_exptrain_sizes
        and antsrl_jointtrain_sizes: 2; antsrl_reworktrain_sizes: 4)."""
        n = C.c_int32()
        self._sizes(B, None, C.byref(n))
        return n.value

    def _loss(self, loss):
        return torch.empty((), dtype=torch.float32, device=self.device) if loss is None else loss

    def _grads(self, grads):
        g = self.grads if grads is None else grads
        assert g.device == self.device and g.dtype == torch.float32 and g.numel() == self.trained_floats and g.is_contiguous()
        return g

    def train(self, replay, done: bool, minibatch: Optional[int] = None, min_replay: int = 1000,
              generator: Optional[torch.Generator] = None):
        """The reference's train: 0 below min_replay, else a step on `minibatch` rows (the class's by default) drawn on
        the device (with replacement), then the target counter (host side: `done` is a host bool) and the sync."""
        if len(replay) < min_replay:
            return 0
        idx = torch.randint(0, len(replay), (self.minibatch if minibatch is None else minibatch,), device=self.device,
                            generator=generator)
        return self.train_on(replay, idx, done)

    def train_on(self, batch_or_replay, idx: Optional[torch.Tensor], done: bool):
        """train() on rows the caller picked: the step, then the target counter and the sync."""
        loss = self.step(batch_or_replay, idx)
        self._count_target(done)
        return loss


class _MemoryBlocks:
    """A memory net's state buffer (include/antsrl.h, antsrl_memtrain_sizes) seen from the host, for MemoryTrainer and
    for every member of population.PopulationMemoryTrainer: the sizes, the tensors' offsets in the flat parameter block
    and the views on a buffer's parameters and Adam moments.  Needs `_lib` and `device`."""

    def _init_blocks(self, shape, n_features: int, power: int, mem_size: int, n_rot: int, n_ph: int) -> None:
        self.shape = shape
        self.power, self.mem_size, self.n_rot, self.n_ph = power, mem_size, n_rot, n_ph
        pf, tf, sb = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _lib.check(self._lib.antsrl_memtrain_sizes(C.byref(self.shape), 1, C.byref(pf), C.byref(tf), C.byref(sb), None),
                   "memtrain_sizes")
        self.params_floats, self.trained_floats, self.state_bytes = pf.value, tf.value, sb.value
        # the flat layout (include/antsrl.h): state_dict order, dense, weight then bias per layer
        self._offs = {}
        off = 0
        for name, (o, i) in memnet_param_shapes(n_features, power, mem_size, n_rot, n_ph).items():
            self._offs[name + ".weight"] = (off, (o, i))
            off += o * i
            self._offs[name + ".bias"] = (off, (o,))
            off += o
        assert off == self.params_floats

    def _adam_offsets(self):
        """Byte offsets of Adam's m and v in a state buffer (256-byte aligned blocks behind the parameters)."""
        m_off = (self.params_floats * 4 + 255) // 256 * 256
        return m_off, (m_off + self.trained_floats * 4 + 255) // 256 * 256

    def _adam_range(self):
        m_off, v_off = self._adam_offsets()
        return slice(m_off, v_off + self.trained_floats * 4)

    def _views(self, buf, region="params"):
        f = buf.view(torch.float32)
        if region == "params":
            base, names = 0, list(self._offs)
        else:
            m_off, v_off = self._adam_offsets()
            base = (m_off if region == "m" else v_off) // 4
            names = [k for k in self._offs if k.split(".")[0] in TRAINED_LAYERS]
        return {k: f[base + self._offs[k][0]: base + self._offs[k][0] + math.prod(self._offs[k][1])].view(self._offs[k][1])
                for k in names}

    def _init_state(self, sd, states) -> None:
        """antsrl_memtrain_init of every buffer in `states` from the 26 tensors of sd (shapes checked): masters and packs
        from sd, Adam's moments zero."""
        for k, (_, shp) in self._offs.items():
            assert tuple(sd[k].shape) == shp, (k, tuple(sd[k].shape), shp)
        src = {k: torch.as_tensor(sd[k]).to(self.device, torch.float32).contiguous() for k in self._offs}
        ptrs = memnet_param_ptrs(src)
        with torch.cuda.device(self.device):
            for state in states:
                _lib.check(self._lib.antsrl_memtrain_init(C.byref(self.shape), ptrs, _p(state), _lib.stream(self.device)),
                           "memtrain_init")

    def _adam_dict(self, buf, step: int) -> dict:
        """torch.optim.Adam's state for the 18 trained tensors of a buffer: step, exp_avg, exp_avg_sq (copies)."""
        return dict(step=step, exp_avg=_clones(self._views(buf, "m")), exp_avg_sq=_clones(self._views(buf, "v")))


class MemoryTrainer(_MemoryBlocks, _DqnTrainer):
    """CollectAgentMemory's model, target model and optimizer on the device (defaults: the reference class's,
    discount 0.5, lr 1e-4; main.py passes 0.99 and 1e-5).

    `step(batch_or_replay, idx)` is one training step (grad + apply) and returns the loss as a 0-d device tensor;
    `train(replay, done)` is CollectAgentMemory.train (:133-176) with the replay on the device.  `policy` is a
    MemoryPolicy holding the TARGET net (get_action acts with the target net, :194), repacked at every sync_target() in
    `policy_precision` ("bf16" or "fp32", MemoryPolicy's precision); the training step itself has bf16 operands either
    way."""

    def __init__(self, n_features: int, device, discount: float = 0.5, lr: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, update_target_every: int = 1, power: int = 5, mem_size: int = 20, n_rot: int = 3,
                 n_ph: int = 3, seed: int = 0, state_dict=None, policy_precision: str = "bf16"):
        if state_dict is not None:
            shp = memnet_shape_from_state_dict(state_dict)
            assert shp["n_features"] == n_features, "state_dict is for %d features, not %d" % (shp["n_features"], n_features)
            power, mem_size, n_rot, n_ph = shp["power"], shp["mem_size"], shp["n_rot"], shp["n_ph"]
        super().__init__(n_features, device, 2 + mem_size, discount, lr, betas, eps, update_target_every)
        self.policy = MemoryPolicy(n_features, self.device, power=power, mem_size=mem_size, n_rot=n_rot, n_ph=n_ph,
                                   seed=seed, precision=policy_precision)
        if state_dict is None:
            state_dict = {k: v.clone() for k, v in self.policy.state_dict().items()}
        self._init_blocks(self.policy.shape, n_features, power, mem_size, n_rot, n_ph)
        self._model = torch.empty((self.state_bytes,), dtype=torch.uint8, device=self.device)  # 512-byte aligned blocks
        self._target = torch.empty_like(self._model)
        self.grads = torch.zeros((self.trained_floats,), dtype=torch.float32, device=self.device)
        self.load_state_dict(state_dict, _reset_adam=True)

    # ---- weights ------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """The model net's 26 tensors (copies), the reference's names and order."""
        return _clones(self._views(self._model))

    def target_state_dict(self) -> dict:
        return _clones(self._views(self._target))

    def load_state_dict(self, sd, _reset_adam: bool = False) -> None:
        """CollectAgentMemory.load_model (:213-215): sets the model AND the target net (and the acting policy).  Adam's
        state is kept, as the reference's optimizer keeps it."""
        keep = None if _reset_adam else self._model[self._adam_range()].clone()
        self._init_state(sd, (self._model, self._target))
        if keep is not None:
            self._model[self._adam_range()] = keep
        self._repack_policy()

    def adam_state(self) -> dict:
        """torch.optim.Adam's state for the 18 trained tensors: step, exp_avg, exp_avg_sq (copies)."""
        return self._adam_dict(self._model, self.step_count)

    def grad_dict(self, grads: Optional[torch.Tensor] = None) -> dict:
        """The flat gradient (self.grads by default) as views named like the 18 trained state_dict tensors."""
        g = self.grads if grads is None else grads
        return {k: g[o: o + math.prod(shp)].view(shp) for k, (o, shp) in self._offs.items() if k.split(".")[0] in TRAINED_LAYERS}

    def _repack_policy(self):
        """policy := target net (a copy into the policy's own tensors, then antsrl_memnet_pack_ex in its precision)."""
        tv = self._views(self._target)
        for k, dst in self.policy.params.items():
            dst.copy_(tv[k])
        ptrs = memnet_param_ptrs(self.policy.params)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_memnet_pack_ex(C.byref(self.shape), self.policy._precision_id(), ptrs,
                                                       _p(self.policy.packed), _lib.stream(self.device)),
                       "memnet_pack_ex")

    def sync_target(self) -> None:
        """target := model (:170-174), and the acting policy with it.  Adam's state is not copied."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_memtrain_copy(C.byref(self.shape), _p(self._model), _p(self._target),
                                                      _lib.stream(self.device)), "memtrain_copy")
        self._repack_policy()
        self.syncs += 1

    # ---- the two stages -----------------------------------------------------------------------------------------
    def _sizes(self, B, workspace_bytes, launches):
        assert launches is None, "antsrl_memtrain_sizes reports no launch count"
        _lib.check(self._lib.antsrl_memtrain_sizes(C.byref(self.shape), B, None, None, None, workspace_bytes), "memtrain_sizes")

    def grad(self, batch_or_replay, idx: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Stage 1: the loss (0-d device tensor) and the gradients of the 18 trained tensors into self.grads.  Rows are
        idx (int64 on the device, values in [0, len)) of a DeviceReplayMemory or of a 7-tuple of arrays (states,
        agent_states, actions, rewards, new_states, new_agent_states, dones), or all rows when idx is None."""
        (st, ast, act, rw, nst, nast, dn), _, B = self._batch(batch_or_replay, idx)
        loss = self._loss(loss)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_memtrain_grad(C.byref(self.shape), _p(self._model), _p(self._target), _p(st), _p(ast),
                                                      _p(act), _p(rw), _p(nst), _p(nast), _p(dn), _p(idx), B, self.discount,
                                                      _p(self.grads), _p(loss), _p(self._work), _lib.stream(self.device)),
                       "memtrain_grad")
        return loss

    def apply(self, grads: Optional[torch.Tensor] = None) -> None:
        """Stage 2: one Adam step over the flat gradient (self.grads by default), then the bf16 repack."""
        g = self._grads(grads)
        self.step_count += 1
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_memtrain_apply(C.byref(self.shape), _p(self._model), _p(g), self.step_count, self.lr,
                                                       self.betas[0], self.betas[1], self.eps, _lib.stream(self.device)),
                       "memtrain_apply")

    def step(self, batch_or_replay, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step on the minibatch (grad, then apply): returns the loss as a 0-d device tensor."""
        loss = self.grad(batch_or_replay, idx)
        self.apply()
        return loss


class _FlatTrainer(_DqnTrainer):
    """What the linear, the explore, the joint and the rework trainer share on top of _DqnTrainer: their entries antsrl_<entry>_sizes
    / _grad / _apply / _step take one argument order behind the net's own leading arguments (include/antsrl.h), so the
    three stages and `_sizes` are written once.  A subclass names its `entry`, gives `_net()` (what _grad and _step take
    in front of the arrays), keeps Adam's moments in `_adam` [2][P] (`_alloc_trained`) and overrides `_weights_changed`
    when a training step moves its acting weights, `_lead()` when its entries' leading argument is not n_features, and
    `_apply_net()` (what _apply takes in front of Adam's m) when its net is not one block `model`.

    sync_target and load_state_dict are written once too: a subclass gives `_copy_target()`, what its target net owns
    following the model, and `_rename(sd)`, a state_dict under the names of its views.  `version` counts the changes of
    the acting weights: it moves behind the copy.

    The views are those of a net that is ONE flat block described by `_offs` (name -> (offset, shape)), `model` and
    `target`: the explore and the rework trainer's (the joint trainer's `model`; its target is layer3 alone).  The linear
    trainer's net has two parts and it writes its own."""

    entry = None  # "lintrain", "exptrain", "jointtrain", "reworktrain"

    def _net(self) -> tuple:
        raise NotImplementedError

    def _lead(self):
        """The leading argument of every entry."""
        return self.n_features

    def _apply_net(self) -> tuple:
        return self._lead(), _p(self.model)

    def _sizes(self, B, workspace_bytes, launches):
        name = "%s_sizes" % self.entry
        _lib.check(getattr(self._lib, "antsrl_" + name)(self._lead(), B, None, workspace_bytes, launches), name)

    def _copy_target(self) -> None:
        raise NotImplementedError

    @staticmethod
    def _rename(sd):
        return sd

    def _alloc_trained(self, trained_floats: int) -> None:
        """Adam's moments and the gradient of the trained floats, zeroed, and `version` at 0."""
        self.trained_floats = trained_floats
        self.version = 0
        self._adam = torch.zeros((2, trained_floats), dtype=torch.float32, device=self.device)
        self.grads = torch.zeros((trained_floats,), dtype=torch.float32, device=self.device)

    def _weights_changed(self) -> None:
        """A call that changed the model's weights has been enqueued."""

    def _call(self, stage: str, *args):
        name = "%s_%s" % (self.entry, stage)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, "antsrl_" + name)(*args, _lib.stream(self.device)), name)

    def _adam_args(self) -> tuple:
        return self.step_count, self.lr, self.betas[0], self.betas[1], self.eps

    # ---- weights ------------------------------------------------------------------------------------------------
    def _views(self, flat) -> dict:
        return {k: flat[o: o + math.prod(shp)].view(shp) for k, (o, shp) in self._offs.items()}

    def _model_views(self) -> dict:
        return self._views(self.model)

    def state_dict(self) -> dict:
        """The model's tensors (copies) under the reference's names, in its order."""
        return _clones(self._model_views())

    def target_state_dict(self) -> dict:
        return _clones(self._views(self.target))

    def load_state_dict(self, sd) -> None:
        """The reference's load_model: sets the model AND the target net (the subclass says under which names, and what
        else follows).  Adam's state is kept, as the reference's optimizer keeps it."""
        copy_named(self._rename(sd), self._model_views())
        self._copy_target()
        self.version += 1

    def sync_target(self) -> None:
        """target := model, as the subclass's _copy_target has it.  Adam's state is not copied."""
        self._copy_target()
        self.syncs += 1
        self.version += 1

    def adam_state(self) -> dict:
        """torch.optim.Adam's state for the trained tensors: step, exp_avg, exp_avg_sq (copies)."""
        return dict(step=self.step_count, exp_avg=_clones(self._views(self._adam[0])),
                    exp_avg_sq=_clones(self._views(self._adam[1])))

    def grad_dict(self, grads: Optional[torch.Tensor] = None) -> dict:
        """The flat gradient (self.grads by default) as views named like the trained tensors."""
        return self._views(self.grads if grads is None else grads)

    # ---- the stages ---------------------------------------------------------------------------------------------
    def grad(self, batch_or_replay, idx: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The loss (0-d device tensor) and the gradients of the trained floats into self.grads; nothing is updated.
        Rows: as MemoryTrainer.grad."""
        arrays, N, B = self._batch(batch_or_replay, idx)
        loss = self._loss(loss)
        self._call("grad", *self._net(), *map(_p, arrays), N, _p(idx), B, self.discount, _p(self.grads), _p(loss),
                   _p(self._work))
        return loss

    def apply(self, grads: Optional[torch.Tensor] = None) -> None:
        """One Adam step on the trained floats from the flat gradient (self.grads by default)."""
        g = self._grads(grads)
        self.step_count += 1
        self._call("apply", *self._apply_net(), _p(self._adam[0]), _p(self._adam[1]), _p(g), *self._adam_args())
        self._weights_changed()

    def step(self, batch_or_replay, idx: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None,
             keep_grads: bool = True) -> torch.Tensor:
        """One training step on the minibatch, gradient and Adam in the same launches (antsrl_<entry>_step): returns the
        loss as a 0-d device tensor.  The same bits as grad() followed by apply()."""
        arrays, N, B = self._batch(batch_or_replay, idx)
        loss = self._loss(loss)
        self.step_count += 1
        self._call("step", *self._net(), _p(self._adam[0]), _p(self._adam[1]), *map(_p, arrays), N, _p(idx), B, self.discount,
                   *self._adam_args(), _p(self.grads) if keep_grads else None, _p(loss), _p(self._work))
        self._weights_changed()
        return loss


#: CollectModel.state_dict()'s names and order (agents/collect_agent.py:24-51 over explore_agent_pytorch.py:24-45)
LINEAR_NAMES = ("explore_model.layer1.weight", "explore_model.layer1.bias", "explore_model.layer2.weight",
                "explore_model.layer2.bias", "layer3.weight", "layer3.bias")
#: the four trained tensors in the flat 198-float block (include/antsrl.h): name -> (offset, shape)
LINEAR_TRAINED = {"explore_model.layer2.weight": (0, (3, 32)), "explore_model.layer2.bias": (96, (3,)),
                  "layer3.weight": (99, (3, 32)), "layer3.bias": (195, (3,))}


#: ExploreModel.state_dict()'s names and order (agents/explore_agent_pytorch.py:24-45)
EXPLORE_NAMES = ("layer1.weight", "layer1.bias", "layer2.weight", "layer2.bias")


def collect_names(sd) -> dict:
    """sd under CollectModel's names: ExploreModel's bare layer1 / layer2 go behind the `explore_model.` prefix."""
    return {(k if (k.startswith("explore_model.") or k.startswith("layer3.")) else "explore_model." + k): v for k, v in sd.items()}


def explore_names(sd) -> dict:
    """sd under ExploreModel's bare names: CollectModel's `explore_model.` prefix goes."""
    return {(k[len("explore_model."):] if k.startswith("explore_model.") else k): v for k, v in sd.items()}


def linear_trained_views(flat) -> dict:
    """The four trained tensors as views of a flat 198-float block: the heads, a row of Adam's moments, a gradient."""
    return {k: flat[o: o + math.prod(shp)].view(shp) for k, (o, shp) in LINEAR_TRAINED.items()}


def linear_model_views(w1, b1, heads) -> dict:
    """The linear net's six tensors under CollectModel's names, in its order: views of layer1 and of the heads' block."""
    return {"explore_model.layer1.weight": w1, "explore_model.layer1.bias": b1, **linear_trained_views(heads)}


def linear_l3_views(target_l3) -> dict:
    """layer3 as views of the target net's only own tensor, its 99-float copy."""
    return {"layer3.weight": target_l3[0:96].view(3, 32), "layer3.bias": target_l3[96:99]}


def linear_target_state_dict(state_dict: dict, target_l3) -> dict:
    """The target net's state_dict from the model's: the shared layer1 and layer2, its own layer3 (a copy)."""
    return {**state_dict, **_clones(linear_l3_views(target_l3))}


def linear_adam_state(step: int, adam) -> dict:
    """torch.optim.Adam's state for the four trained tensors from the moments [2][198]: step, exp_avg, exp_avg_sq (copies)."""
    return dict(step=step, exp_avg=_clones(linear_trained_views(adam[0])), exp_avg_sq=_clones(linear_trained_views(adam[1])))


class _CollectTrainer(_FlatTrainer):
    """What the linear and the joint trainer share: CollectModel's two nets share one ExploreModel, so layer1 and layer2
    are live in both and the target net owns layer3 alone, `target_l3` (99 floats).  load_state_dict is
    CollectAgent.load_model (agents/collect_agent.py:182-184) and takes CollectModel's names, or ExploreModel's bare
    layer1 / layer2 (with layer3)."""

    _rename = staticmethod(collect_names)

    def target_state_dict(self) -> dict:
        """The target net's: the shared layer1 and layer2, its own layer3."""
        return linear_target_state_dict(self.state_dict(), self.target_l3)

    def load_explore_state_dict(self, sd) -> None:
        """The hand-over from stage 1 of the curriculum (the line agents/collect_agent.py:84 has commented out): layer1
        and layer2 from a four-tensor ExploreModel state_dict (an ExploreAgent's save_model; bare names or behind the
        `explore_model.` prefix).  layer3, its target copy and Adam's state stay as they are."""
        copy_named(collect_names(sd), self._model_views(), LINEAR_NAMES[:4])
        self.version += 1


class LinearTrainer(_CollectTrainer):
    """CollectAgent's model, target model and optimizer on the device (agents/collect_agent.py:54-148; defaults: the
    reference class's, discount 0.5, Adam lr 1e-4), trained by `antsrl_lintrain_step` (antsrl_lintrain.hip).

    Only layer2 and layer3 are trained (198 floats): the reference freezes layer1, whose .grad stays None.  Model and
    target net share one ExploreModel, so the target net's rotation head is the live layer2 and only layer3 has a target
    copy.  `policy` is the acting LinearPolicy (get_action acts with the target net, :166): the shared layer1, the live
    layer2 and the target layer3 — its head tensors are views of this trainer's buffers, so it needs no copy after a
    step.  `version` counts the changes of the acting weights (every step moves layer2).

    The surface is MemoryTrainer's: grad / apply / step, train(replay, done), state_dict / load_state_dict under the
    reference's six names, target_state_dict, sync_target, adam_state, grad_dict.  train() is CollectAgent.train
    (:105-148)."""

    entry = "lintrain"

    def __init__(self, n_features: int, device, discount: float = 0.5, lr: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, update_target_every: int = 1, seed: int = 0, state_dict=None):
        from .policy import LinearPolicy
        super().__init__(n_features, device, 2, discount, lr, betas, eps, update_target_every)
        self._alloc_trained(198)
        p = LinearPolicy(n_features, self.device, seed=seed)
        self.heads = torch.cat([p.w2.reshape(-1), p.b2, p.w3.reshape(-1), p.b3]).contiguous()
        self.target_l3 = self.heads[99:198].clone()
        p.w2, p.b2 = self.heads[0:96].view(3, 32), self.heads[96:99]              # the live layer2
        p.w3, p.b3 = linear_l3_views(self.target_l3).values()                     # the target layer3
        self.policy = p
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- weights ------------------------------------------------------------------------------------------------
    def _model_views(self) -> dict:
        return linear_model_views(self.policy.w1, self.policy.b1, self.heads)

    def _copy_target(self) -> None:
        """target := model (:143-146): layer3 is all the two nets do not share."""
        self.target_l3.copy_(self.heads[99:198])

    def adam_state(self) -> dict:
        """torch.optim.Adam's state for the four trained tensors: step, exp_avg, exp_avg_sq (copies)."""
        return linear_adam_state(self.step_count, self._adam)

    def grad_dict(self, grads: Optional[torch.Tensor] = None) -> dict:
        """The flat gradient (self.grads by default) as views named like the four trained tensors."""
        return linear_trained_views(self.grads if grads is None else grads)

    # ---- the stages ---------------------------------------------------------------------------------------------
    def _net(self) -> tuple:
        p = self.policy
        return self.n_features, _p(p.w1), _p(p.b1), _p(self.heads), _p(self.target_l3)

    def _apply_net(self) -> tuple:
        return (_p(self.heads),)

    def _weights_changed(self) -> None:
        self.version += 1  # every step moves the live layer2


class ExploreTrainer(_FlatTrainer):
    """ExploreAgentPytorch's model, target model and optimizer on the device (agents/explore_agent_pytorch.py:48-133 as it
    was meant: ExploreModel with the concat of CollectModel.forward, collect_agent.py:47-49; defaults: the reference
    class's, discount 0.5, Adam lr 1e-4), trained by `antsrl_exptrain_step` (antsrl_exptrain.hip).

    Both layers are trained: one flat fp32 block of P = 32 (F + 2) + 32 + 96 + 3 floats per net (include/antsrl.h), the
    target net a second block.  `policy` is the acting LinearPolicy without a pheromone head (get_action acts with the
    target net, :150): its w1, b1, w2, b2 are views of the TARGET block, so a training step never changes the actions and
    a sync needs no copy into the policy.  `version` counts the changes of the acting weights: syncs and loads.

    The surface is LinearTrainer's: grad / apply / step, train(replay, done), train_on, launches, state_dict /
    load_state_dict under ExploreModel's four names, target_state_dict, sync_target, adam_state, grad_dict.  train() is
    ExploreAgentPytorch.train (:90-133)."""

    minibatch = 256
    entry = "exptrain"

    def __init__(self, n_features: int, device, discount: float = 0.5, lr: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, update_target_every: int = 1, seed: int = 0, state_dict=None):
        from .policy import LinearPolicy
        super().__init__(n_features, device, 2, discount, lr, betas, eps, update_target_every)
        IN = n_features + 2
        self._offs = {"layer1.weight": (0, (32, IN)), "layer1.bias": (32 * IN, (32,)),
                      "layer2.weight": (32 * IN + 32, (3, 32)), "layer2.bias": (32 * IN + 128, (3,))}
        tf = C.c_size_t()
        _lib.check(self._lib.antsrl_exptrain_sizes(n_features, 1, C.byref(tf), None, None), "exptrain_sizes")
        assert tf.value == 32 * IN + 131
        self._alloc_trained(tf.value)
        p = LinearPolicy(n_features, self.device, with_pheromone_head=False, seed=seed)
        self.model = torch.cat([p.w1.reshape(-1), p.b1, p.w2.reshape(-1), p.b2]).contiguous()
        self.target = self.model.clone()
        tv = self._views(self.target)
        p.w1, p.b1, p.w2, p.b2 = (tv[k] for k in EXPLORE_NAMES)  # the acting net IS the target block
        self.policy = p
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- weights ------------------------------------------------------------------------------------------------
    #: load_state_dict is ExploreAgentPytorch.load_model (:157-159) and takes ExploreModel's names, bare or behind
    #: CollectModel's `explore_model.` prefix (other entries, such as layer3, are ignored)
    _rename = staticmethod(explore_names)

    def _copy_target(self) -> None:
        """target := model (:127-131): one device copy of the block; the acting policy's tensors are views of it."""
        self.target.copy_(self.model)

    # ---- the stages ---------------------------------------------------------------------------------------------
    def _net(self) -> tuple:
        return self.n_features, _p(self.model), _p(self.target)


class JointTrainer(_CollectTrainer):
    """CollectAgent's model, target model and optimizer on the device with the freeze of layer1 lifted and nothing else
    changed: the third stage of the linear agent's curriculum, trained by `antsrl_jointtrain_step`
    (antsrl_jointtrain.hip).  It is the reference's own train() (agents/collect_agent.py:105-148) once
    requires_grad is set again on explore_model.layer1: the reference's Adam already holds all six tensors.

    All six tensors are trained: ONE flat fp32 block `model` of P = 32 (F + 2) + 32 + 198 floats in
    CollectModel.state_dict()'s order (include/antsrl.h).  Model and target net share one ExploreModel, so layer1 and
    layer2 are live in both nets and only layer3 has a target copy, `target_l3` (99 floats).  `policy` is the acting
    LinearPolicy (get_action acts with the target net, :166): its w1, b1, w2, b2 are views of `model` and its w3, b3 views
    of `target_l3`, so it needs no copy after a step.  `version` counts the changes of the acting weights: every step
    moves layer1 and layer2.

    The surface is LinearTrainer's: grad / apply / step, train(replay, done), train_on, launches, state_dict /
    load_state_dict under the reference's six names, load_explore_state_dict, target_state_dict, sync_target,
    adam_state, grad_dict."""

    entry = "jointtrain"

    def __init__(self, n_features: int, device, discount: float = 0.5, lr: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, update_target_every: int = 1, seed: int = 0, state_dict=None):
        from .policy import LinearPolicy
        super().__init__(n_features, device, 2, discount, lr, betas, eps, update_target_every)
        IN = n_features + 2
        shapes = ((32, IN), (32,), (3, 32), (3,), (3, 32), (3,))
        self._offs, off = {}, 0
        for k, shp in zip(LINEAR_NAMES, shapes):
            self._offs[k] = (off, shp)
            off += math.prod(shp)
        tf = C.c_size_t()
        _lib.check(self._lib.antsrl_jointtrain_sizes(n_features, 1, C.byref(tf), None, None), "jointtrain_sizes")
        assert tf.value == off == 32 * IN + 230
        self._alloc_trained(tf.value)
        p = LinearPolicy(n_features, self.device, seed=seed)
        self.model = torch.cat([t.reshape(-1) for t in (p.w1, p.b1, p.w2, p.b2, p.w3, p.b3)]).contiguous()
        self._l3 = slice(self._offs["layer3.weight"][0], off)  # layer3 in the block: the 99 floats the target copies
        self.target_l3 = self.model[self._l3].clone()
        mv = self._views(self.model)
        p.w1, p.b1, p.w2, p.b2 = (mv[k] for k in LINEAR_NAMES[:4])                # the live layer1 and layer2
        p.w3, p.b3 = linear_l3_views(self.target_l3).values()                     # the target layer3
        self.policy = p
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # ---- weights ------------------------------------------------------------------------------------------------
    def _copy_target(self) -> None:
        """target := model (:143-146): layer3 is all the two nets do not share."""
        self.target_l3.copy_(self.model[self._l3])

    # ---- the stages ---------------------------------------------------------------------------------------------
    def _net(self) -> tuple:
        return self.n_features, _p(self.model), _p(self.target_l3)

    def _weights_changed(self) -> None:
        self.version += 1  # every step moves the live layer1 and layer2


class ReworkTrainer(_FlatTrainer):
    """CollectAgentRework's model, target model and optimizer on the device (agents/collect_agent_rework.py:66-152;
    defaults: the reference class's, discount 0.5, Adam lr 1e-4, minibatch 264), trained by `antsrl_reworktrain_step`
    (antsrl_reworktrain.hip).

    All ten layers are trained: one flat fp32 block of P floats per net (include/antsrl.h), the 20 state_dict tensors in
    their order; the target net is a second block.  `policy` is the acting ReworkPolicy (get_action acts with the target
    net, :170): its tensors are views of the TARGET block and its collapsed buffer is the one the training step takes
    its TD targets from.  sync_target and load_state_dict copy the block and collapse once; a training step changes
    neither the policy's collapsed buffer nor `version`, which counts the changes of the acting weights.

    The surface is ExploreTrainer's: grad / apply / step, train(replay, done), train_on, launches, state_dict /
    load_state_dict under CollectModelRework's twenty names (the hidden widths come from a state_dict's shapes),
    target_state_dict, sync_target, adam_state, grad_dict."""

    entry = "reworktrain"

    def __init__(self, n_features: int, device, discount: float = 0.5, lr: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, update_target_every: int = 1, n_rot: int = 3, n_ph: int = 3, seed: int = 0,
                 state_dict=None):
        from .policy import ReworkPolicy, rework_param_shapes, rework_shape_from_state_dict
        super().__init__(n_features, device, 2, discount, lr, betas, eps, update_target_every)
        if state_dict is None:
            state_dict = ReworkPolicy(n_features, "cpu", n_rot=n_rot, n_ph=n_ph, seed=seed).state_dict()
        shp = rework_shape_from_state_dict(state_dict)
        assert shp["n_features"] == n_features, "state_dict is for %d features, not %d" % (shp["n_features"], n_features)
        self.n_rot, self.n_ph = shp["n_rot"], shp["n_ph"]
        self.shape = _lib.AntsReworkShape(*[shp[n] for n, _ in _lib.AntsReworkShape._fields_])
        self._offs, off = {}, 0
        for name, (o, i) in rework_param_shapes(**{k: v for k, v in shp.items() if k != "agent_dim"}).items():
            self._offs[name + ".weight"] = (off, (o, i))
            self._offs[name + ".bias"] = (off + o * i, (o,))
            off += o * i + o
        pf = C.c_size_t()
        _lib.check(self._lib.antsrl_reworktrain_sizes(C.byref(self.shape), 1, C.byref(pf), None, None), "reworktrain_sizes")
        assert pf.value == off
        self._alloc_trained(pf.value)
        self.model = torch.cat([torch.as_tensor(state_dict[k]).to(torch.float32).reshape(-1) for k in self._offs]).to(self.device)
        self.target = self.model.clone()
        self.policy = ReworkPolicy(n_features, self.device, params=self._views(self.target))  # acts on the target block

    # ---- weights ------------------------------------------------------------------------------------------------
    def _copy_target(self) -> None:
        """target := model (:147-150, and in CollectAgentRework.load_model, :186-188, which load_state_dict is): one
        device copy of the block, then one collapse of it; the acting policy's tensors are views of the block."""
        self.target.copy_(self.model)
        self.policy.recollapse()

    # ---- the stages ---------------------------------------------------------------------------------------------
    def _lead(self):
        return C.byref(self.shape)

    def _net(self) -> tuple:
        return self._lead(), _p(self.model), _p(self.policy.collapsed)
