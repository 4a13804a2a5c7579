"""In-loop policy inference on the GPU (BASELINE config 5).

`LinearPolicy` holds the weights of the reference's DQN nets — `ExploreModel`
(agents/explore_agent_pytorch.py:24-45: layer1 Linear(F+2 -> 32), layer2 Linear(32 -> 3)) plus the
pheromone head `CollectModel.layer3` (agents/collect_agent.py:24-51) — and evaluates them on the
observation tensor with the bf16 MFMA kernel `antsrl_policy_mlp` (no torch matmul, no copy of the
observation): rotation = argmax(layer2(out)) - 1, pheromone = argmax(layer3(out)), as
agents/collect_agent_memory.py:196-199 does on the host.

The reference's checkpoints (agents/models/*.h5) are stale against its current code (150-wide
inputs), so weights are random-initialised like nn.Linear, or loaded from any
state_dict with layer1/layer2/(layer3) of the right shapes.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import ptr as _p


def linear_init(shapes: dict, seed: int) -> dict:
    """nn.Linear's default initialisation (kaiming_uniform(a=sqrt(5)) == U(-1/sqrt(in), 1/sqrt(in)), the bias from the
    same interval) of the layers name -> (out, in), as a state_dict on the CPU: one generator seeded once, the layers in
    the dict's order, a layer's weight drawn before its bias."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    sd = {}
    for name, (out_f, in_f) in shapes.items():
        b = 1.0 / math.sqrt(in_f)
        sd[name + ".weight"] = (torch.rand((out_f, in_f), generator=g) * 2 - 1) * b
        sd[name + ".bias"] = (torch.rand((out_f,), generator=g) * 2 - 1) * b
    return sd


def check_rows(n_features: int, obs: torch.Tensor, agent_state: torch.Tensor, env) -> tuple:
    """What every act path checks of its rows: obs [..., P, P, K] (float32, or bfloat16 as `env` produced it) and
    agent_state float32 [..., 2], dense -> (the leading shape, the rows)."""
    lead = obs.shape[:-3]
    m = math.prod(lead)
    assert obs.is_contiguous() and agent_state.is_contiguous()
    assert obs.dtype in (torch.float32, torch.bfloat16) and agent_state.dtype == torch.float32
    if env is not None:
        assert env.obs.dtype == obs.dtype, "obs and env.obs differ in dtype"
    assert obs.numel() == m * n_features and agent_state.numel() == m * 2
    return lead, m


class LinearPolicy:
    def __init__(self, n_features: int, device, with_pheromone_head: bool = True, seed: int = 0):
        shapes = dict(layer1=(32, n_features + 2), layer2=(3, 32))
        if with_pheromone_head:
            shapes["layer3"] = (3, 32)
        sd = {k: v.to(device).contiguous() for k, v in linear_init(shapes, seed).items()}
        self.n_features = n_features
        self.device = torch.device(device)
        self.w1, self.b1 = sd["layer1.weight"], sd["layer1.bias"]
        self.w2, self.b2 = sd["layer2.weight"], sd["layer2.bias"]
        self.w3, self.b3 = sd.get("layer3.weight"), sd.get("layer3.bias")
        self._lib = _lib.load()
        self._rot = self._ph = None

    def load_state_dict(self, sd) -> None:
        """Accepts the reference's parameter names: layer1 / layer2 / layer3 .weight / .bias as `ExploreModel.state_dict()`
        has them (explore_agent_pytorch.py:36-37) or behind the `explore_model.` prefix of `CollectModel.state_dict()`
        (collect_agent.py:28,44)."""
        sd = {(k[len("explore_model."):] if k.startswith("explore_model.") else k): v for k, v in sd.items()}
        for name, attr in (("layer1", "1"), ("layer2", "2"), ("layer3", "3")):
            if name + ".weight" in sd:
                w = torch.as_tensor(sd[name + ".weight"]).to(self.device, torch.float32).contiguous()
                b = torch.as_tensor(sd[name + ".bias"]).to(self.device, torch.float32).contiguous()
                assert w.shape == getattr(self, "w" + attr).shape, "%s: %s" % (name, tuple(w.shape))
                setattr(self, "w" + attr, w)
                setattr(self, "b" + attr, b)

    def act(self, obs: torch.Tensor, agent_state: torch.Tensor, logits: Optional[torch.Tensor] = None, env=None):
        """obs [..., P, P, K] (float32, or bfloat16 from a BatchedAntsEnv(obs_dtype=torch.bfloat16) passed as
        `env`) and agent_state float32 [..., 2] on the GPU -> (rotation int8 [...], pheromone int8 [...] or
        None), ready to pass to step()."""
        lead, m = check_rows(self.n_features, obs, agent_state, env)
        assert obs.dtype != torch.bfloat16 or env is not None, "bfloat16 observations: pass the env that produced them"
        handle = env._h if obs.dtype == torch.bfloat16 else None
        if self._rot is None or self._rot.numel() != m:
            self._rot = torch.empty((m,), dtype=torch.int8, device=self.device)
            self._ph = torch.empty((m,), dtype=torch.int8, device=self.device) if self.w3 is not None else None

        with torch.cuda.device(self.device):
            st = _lib.stream(self.device)
            _lib.check(self._lib.antsrl_policy_mlp(handle, _p(obs), _p(agent_state), m, self.n_features, _p(self.w1),
                                                   _p(self.b1), _p(self.w2), _p(self.b2), _p(self.w3), _p(self.b3),
                                                   _p(self._rot), _p(self._ph), _p(logits), st), "policy_mlp")
        rot = self._rot.view(lead)
        return rot, (self._ph.view(lead) if self._ph is not None else None)

    def attach(self, env) -> None:
        """In-loop form (antsrl_set_inloop_policy): from now on every observation `env` writes also leaves the net's
        actions for the NEXT step in `env.next_rotation` / `env.next_pheromone` (int8 [E, N]) — the values act() returns
        for that observation, computed inside the observation kernel.  Needs bfloat16 observations on the cell-meta
        path; detach() switches it off."""
        assert env.obs.dtype == torch.bfloat16, "the in-loop policy reads bfloat16 observation rows"
        E, N = env.cfg.n_envs, env.cfg.n_ants
        env.next_rotation = torch.zeros((E, N), dtype=torch.int8, device=self.device)
        env.next_pheromone = torch.zeros((E, N), dtype=torch.int8, device=self.device) if self.w3 is not None else None

        with torch.cuda.device(self.device):
            st = _lib.stream(self.device)
            _lib.check(self._lib.antsrl_set_inloop_policy(env._h, self.n_features, _p(self.w1), _p(self.b1), _p(self.w2), _p(self.b2),
                                                          _p(self.w3), _p(self.b3), _p(env.next_rotation), _p(env.next_pheromone), st),
                       "set_inloop_policy")
        env._loaded = "given an in-loop policy"

    def detach(self, env) -> None:
        _lib.check(self._lib.antsrl_set_inloop_policy(env._h, self.n_features, None, None, None, None, None, None, None, None, None),
                   "set_inloop_policy")


#: CollectModelMemory's parameters in its state_dict order (agents/collect_agent_memory.py:39-55): the order
#: antsrl_memnet_pack takes them in
MEMNET_LAYERS = ("layer1", "layer2", "layer3", "layer4", "rotation_layer1", "rotation_layer2", "rotation_layer3",
                 "pheromone_layer1", "pheromone_layer2", "memory_layer1", "memory_layer2", "memory_layer3", "forget_layer")


def memnet_param_ptrs(sd):
    """The 26 device tensors of a CollectModelMemory state_dict as the ABI's `params` array."""
    return (C.c_void_p * 26)(*[sd["%s.%s" % (l, w)].data_ptr() for l in MEMNET_LAYERS for w in ("weight", "bias")])


#: MemoryPolicy precisions -> include/antsrl.h ANTSRL_MEMNET_BF16 / ANTSRL_MEMNET_FP32
MEMNET_PRECISIONS = {"bf16": 0, "fp32": 1}


def memnet_shape_from_state_dict(sd) -> dict:
    """power, mem_size, n_rot, n_ph and n_features of a CollectModelMemory state_dict, from its shapes alone
    (layer1: h2 x D with h2 = 2^(2+power); memory_layer3: mem_size x h2; D = n_features + 2 + mem_size)."""
    shp = {k: tuple(torch.as_tensor(v).shape) for k, v in sd.items()}
    h2, D = shp["layer1.weight"]
    power = int(round(math.log2(h2))) - 2
    assert h2 == 2 ** (2 + power), "layer1 width %d is not a power of two" % h2
    mem = shp["memory_layer3.weight"][0]
    return dict(power=power, mem_size=mem, n_rot=shp["rotation_layer3.weight"][0], n_ph=shp["pheromone_layer2.weight"][0],
                n_features=D - 2 - mem)


def memnet_param_shapes(n_features: int, power: int, mem_size: int, n_rot: int, n_ph: int) -> dict:
    """name -> (out, in) of every Linear of CollectModelMemory (collect_agent_memory.py:39-55)."""
    D, h1, h2, h3 = n_features + 2 + mem_size, 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power)
    return dict(layer1=(h2, D), layer2=(h3, h2), layer3=(h1, h3), layer4=(D, h1), rotation_layer1=(h2, D),
                rotation_layer2=(h3, h2), rotation_layer3=(n_rot, h3), pheromone_layer1=(h1, D), pheromone_layer2=(n_ph, h1),
                memory_layer1=(h2, D), memory_layer2=(h2, h2), memory_layer3=(mem_size, h2), forget_layer=(mem_size, h2))


def memnet_shape(n_features: int, power: int, mem_size: int, n_rot: int, n_ph: int) -> _lib.AntsMemNetShape:
    """The ABI's shape of CollectModelMemory: agent_dim 2, the three hidden widths from `power`."""
    return _lib.AntsMemNetShape(n_features, 2, mem_size, 2 ** (1 + power), 2 ** (2 + power), 2 ** (3 + power), n_rot, n_ph)


class MemoryPolicy:
    """The reference's recurrent memory agent net `CollectModelMemory` (agents/collect_agent_memory.py:24-78, the net
    main.py's CollectAgentMemory trains) evaluated on the device by `antsrl_policy_memory_ex`.

    `precision` picks the kernel: "bf16" (the default: bf16 MFMA operands, fp32 accumulation) or "fp32" (fp32 operands
    throughout: the reference's own fp32 forward up to summation order, so its actions on near-tied q values too).

    Weights are nn.Linear-initialised (seeded) or loaded with load_state_dict from the reference's own state_dict (its
    parameter names; power and mem_size are inferred from the shapes, so the shipped checkpoints load as they are).
    `memory` is the per-ant recurrent state (float32 [M, mem_size] on the device, zeros when first used and after
    reset_memory()): the reference zeros it once in setup (:111), not per episode."""

    def __init__(self, n_features: int, device, power: int = 5, mem_size: int = 20, n_rot: int = 3, n_ph: int = 3,
                 seed: int = 0, precision: str = "bf16"):
        assert precision in MEMNET_PRECISIONS, "precision must be one of %s, not %r" % (tuple(MEMNET_PRECISIONS), precision)
        self.precision = precision
        self.n_features = n_features
        self.device = torch.device(device)
        sd = linear_init(memnet_param_shapes(n_features, power, mem_size, n_rot, n_ph), seed)
        self._lib = _lib.load()
        self.memory = None
        self._rot = self._ph = None
        self._set(sd, power, mem_size, n_rot, n_ph)

    def _set(self, sd, power, mem_size, n_rot, n_ph):
        self.power, self.mem_size, self.n_rot, self.n_ph = power, mem_size, n_rot, n_ph
        self.params = {k: torch.as_tensor(v).to(self.device, torch.float32).contiguous() for k, v in sd.items()}
        self.shape = memnet_shape(self.n_features, power, mem_size, n_rot, n_ph)
        n = C.c_size_t()
        _lib.check(self._lib.antsrl_memnet_packed_bytes_ex(C.byref(self.shape), self._precision_id(), C.byref(n)),
                   "memnet_packed_bytes_ex")
        if self.memory is not None and self.memory.shape[1] != mem_size:
            self.memory = None
        self.packed = None
        if self.device.type != "cuda":  # weights only (no kernel can run on them)
            return
        # (torch blocks are 512-byte aligned; zeros: the pack kernel writes no byte of the padding between two blocks, and
        # two packs of equal weights are then equal byte for byte)
        self.packed = torch.zeros((n.value,), dtype=torch.uint8, device=self.device)
        ptrs = memnet_param_ptrs(self.params)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_memnet_pack_ex(C.byref(self.shape), self._precision_id(), ptrs,
                                                       _p(self.packed), _lib.stream(self.device)), "memnet_pack_ex")

    def _precision_id(self) -> int:
        return MEMNET_PRECISIONS[self.precision]

    def state_dict(self) -> dict:
        return dict(self.params)

    def load_state_dict(self, sd) -> None:
        """A CollectModelMemory state_dict (the reference's parameter names, e.g. torch.load('good_model.h5') or
        target_model.state_dict()); power, mem_size and the head sizes come from its shapes, then the weights are
        repacked in the policy's precision."""
        shp = memnet_shape_from_state_dict(sd)
        assert shp["n_features"] == self.n_features, "state_dict is for %d features, not %d" % (shp["n_features"], self.n_features)
        want = memnet_param_shapes(self.n_features, shp["power"], shp["mem_size"], shp["n_rot"], shp["n_ph"])
        for name, (o, i) in want.items():
            assert tuple(sd[name + ".weight"].shape) == (o, i) and tuple(sd[name + ".bias"].shape) == (o,), name
        self._set({k: sd[k] for l in MEMNET_LAYERS for k in (l + ".weight", l + ".bias")}, shp["power"], shp["mem_size"],
                  shp["n_rot"], shp["n_ph"])

    def reset_memory(self, n_ants: Optional[int] = None) -> None:
        """Zeros the carried memory (CollectAgentMemory.setup, :111); `n_ants` (re)sizes it."""
        m = n_ants if n_ants is not None else (self.memory.shape[0] if self.memory is not None else None)
        self.memory = None if m is None else torch.zeros((m, self.mem_size), dtype=torch.float32, device=self.device)

    def act(self, obs: torch.Tensor, agent_state: torch.Tensor, memory: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None, env=None, tiles=None):
        """CollectAgentMemory.get_action's network branch (:191-200): obs [..., P, P, K] float32 (or bfloat16 from a
        BatchedAntsEnv(obs_dtype=torch.bfloat16)), agent_state float32 [..., 2] on the device ->
        (rotation int8 [...], pheromone int8 [...], new_memory float32 [M, mem_size]).

        The old memory is `memory`, or `self.memory` when None (zeros on first use).  The new memory goes to `out` when
        given (the old one stays intact: the epsilon branch gives it back to exploring colonies, :204, and
        MemoryAgent(state_memory="carried") records it), else in place over the old one.  What the reference's
        update_replay_memory stores (:182) is NOT the old memory: get_action has overwritten self.previous_memory with
        the new one by then (:194), so agent_states and new_agent_states hold the same, post-action memory
        (antsrl_amd/agent.py).
        `q` (float32 [M, n_rot + n_ph]) receives both heads' outputs.

        `tiles` = (tiles int32 [ceil(M / 32)], n_live int32 [1]), device tensors (e.g. from antsrl_agent_plan): the net is
        evaluated by `antsrl_policy_memory_tiles` on the listed 32-ant tiles only, bit for bit as without the list; the
        other ants' rotation, pheromone, memory and q are NOT written (the returned action tensors are reused buffers:
        the caller owns every element it did not list).  In place, the listed tiles must be distinct."""
        assert self.packed is not None, "MemoryPolicy on %s holds weights only: the kernel needs a GPU device" % self.device
        lead, m = check_rows(self.n_features, obs, agent_state, env)
        if memory is None:
            if self.memory is None or self.memory.shape[0] != m:
                assert self.memory is None, "self.memory holds %d ants, not %d: reset_memory(n_ants)" % (self.memory.shape[0], m)
                self.reset_memory(m)
            memory = self.memory
        assert memory.shape == (m, self.mem_size) and memory.dtype == torch.float32 and memory.is_contiguous()
        dst = memory if out is None else out
        assert dst.shape == (m, self.mem_size) and dst.dtype == torch.float32 and dst.is_contiguous()
        if q is not None:
            assert q.shape == (m, self.n_rot + self.n_ph) and q.dtype == torch.float32 and q.is_contiguous()
        if self._rot is None or self._rot.numel() != m:
            self._rot = torch.empty((m,), dtype=torch.int8, device=self.device)
            self._ph = torch.empty((m,), dtype=torch.int8, device=self.device)

        fmt = 1 if obs.dtype == torch.bfloat16 else 0  # ANTSRL_OBS_BF16 / ANTSRL_OBS_F32
        with torch.cuda.device(self.device):
            if tiles is not None:
                lst, n_live = tiles
                for t, n in ((lst, (m + 31) // 32), (n_live, 1)):
                    assert t.dtype == torch.int32 and t.device == obs.device and t.is_contiguous() and t.numel() >= n, \
                        "tiles = (int32 [ceil(M / 32)], int32 [1]) on the observation's device"
                _lib.check(self._lib.antsrl_policy_memory_tiles(C.byref(self.shape), self._precision_id(), _p(self.packed),
                                                                _p(obs), fmt, _p(agent_state), _p(memory), m, _p(dst),
                                                                _p(self._rot), _p(self._ph), _p(q), _p(lst), _p(n_live),
                                                                _lib.stream(self.device)), "policy_memory_tiles")
                return self._rot.view(lead), self._ph.view(lead), dst
            _lib.check(self._lib.antsrl_policy_memory_ex(C.byref(self.shape), self._precision_id(), _p(self.packed), _p(obs),
                                                         fmt, _p(agent_state), _p(memory), m, _p(dst), _p(self._rot), _p(self._ph),
                                                         _p(q), _lib.stream(self.device)), "policy_memory_ex")
        return self._rot.view(lead), self._ph.view(lead), dst


#: CollectModelRework's layers in its state_dict order (agents/collect_agent_rework.py:36-47): the order
#: antsrl_rework_collapse takes them in
REWORK_LAYERS = ("layer1", "layer2", "layer3", "layer4", "rotation_layer1", "rotation_layer2", "rotation_layer3",
                 "rotation_layer4", "pheromone_layer1", "pheromone_layer2")


def rework_shape_from_state_dict(sd) -> dict:
    """AntsReworkShape's fields of a CollectModelRework state_dict, from its shapes alone (layer1: g1 x D with
    D = n_features + 2), after checking that every layer's input is the width of the layer it is fed from."""
    shp = {k: tuple(torch.as_tensor(v).shape) for k, v in sd.items()}
    out = {l: shp[l + ".weight"][0] for l in REWORK_LAYERS}
    D = shp["layer1.weight"][1]
    s = dict(n_features=D - 2, agent_dim=2, g1=out["layer1"], g2=out["layer2"], g3=out["layer3"], r1=out["rotation_layer1"],
             r2=out["rotation_layer2"], r3=out["rotation_layer3"], p1=out["pheromone_layer1"], n_rot=out["rotation_layer4"],
             n_ph=out["pheromone_layer2"])
    for name, want in rework_param_shapes(**{k: v for k, v in s.items() if k != "agent_dim"}).items():
        assert shp[name + ".weight"] == want and shp[name + ".bias"] == want[:1], \
            "%s: %s / %s, not %s" % (name, shp[name + ".weight"], shp[name + ".bias"], want)
    return s


def rework_param_shapes(n_features: int, n_rot: int = 3, n_ph: int = 3, g1: int = 64, g2: int = 128, g3: int = 32,
                        r1: int = 64, r2: int = 128, r3: int = 32, p1: int = 32) -> dict:
    """name -> (out, in) of every Linear of CollectModelRework (collect_agent_rework.py:36-47; its widths by default)."""
    D = n_features + 2
    return dict(layer1=(g1, D), layer2=(g2, g1), layer3=(g3, g2), layer4=(D, g3), rotation_layer1=(r1, D),
                rotation_layer2=(r2, r1), rotation_layer3=(r3, r2), rotation_layer4=(n_rot, r3), pheromone_layer1=(p1, D),
                pheromone_layer2=(n_ph, p1))


class ReworkPolicy:
    """The reference's `CollectModelRework` (agents/collect_agent_rework.py:24-63, the net main.py's CollectAgentRework
    trains) evaluated on the device.  The net has no activation, so its ten layers are multiplied out once per weight
    change (`antsrl_rework_collapse`, float64, rounded once to fp32: `collapsed_weight` [NQ, D], `collapsed_bias` [NQ],
    NQ = n_rot + n_ph) and `act` is NQ fp32 dot products per ant (`antsrl_policy_rework`).

    Weights are nn.Linear-initialised (seeded) or loaded with load_state_dict from the reference's own state_dict (its
    parameter names, e.g. target_model.state_dict(); the widths come from its shapes)."""

    def __init__(self, n_features: int, device, n_rot: int = 3, n_ph: int = 3, seed: int = 0, params=None):
        """params: the 20 tensors (fp32, contiguous, on `device`, the reference's names) to ADOPT as they are instead of
        initialising: the policy reads them where they lie (ReworkTrainer's target block) and `recollapse()` follows
        their changes."""
        self.n_features = n_features
        self.device = torch.device(device)
        self._lib = _lib.load()
        self._rot = self._ph = None
        if params is not None:
            for t in params.values():
                assert t.device.type == self.device.type and t.dtype == torch.float32 and t.is_contiguous()
            self._set(params)
            assert all(self.params[k] is params[k] for k in self.params), "adopted tensors are not copied"
            return
        self._set(linear_init(rework_param_shapes(n_features, n_rot, n_ph), seed))

    def _set(self, sd):
        shp = rework_shape_from_state_dict(sd)
        assert shp["n_features"] == self.n_features, "state_dict is for %d features, not %d" % (shp["n_features"], self.n_features)
        self.n_rot, self.n_ph = shp["n_rot"], shp["n_ph"]
        self.params = {"%s.%s" % (l, w): torch.as_tensor(sd["%s.%s" % (l, w)]).to(self.device, torch.float32).contiguous()
                       for l in REWORK_LAYERS for w in ("weight", "bias")}
        self.shape = _lib.AntsReworkShape(*[shp[n] for n, _ in _lib.AntsReworkShape._fields_])
        n = C.c_size_t()
        _lib.check(self._lib.antsrl_rework_collapsed_bytes(C.byref(self.shape), C.byref(n)), "rework_collapsed_bytes")
        self.collapsed = None
        if self.device.type != "cuda":  # weights only (no kernel can run on them)
            return
        self.collapsed = torch.empty((n.value // 4,), dtype=torch.float32, device=self.device)
        self.recollapse()

    def recollapse(self) -> None:
        """Multiplies the layers out again, into the same collapsed buffer: after the tensors of `params` changed in
        place."""
        ptrs = (C.c_void_p * 20)(*[t.data_ptr() for t in self.params.values()])
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_rework_collapse(C.byref(self.shape), ptrs, _p(self.collapsed),
                                                        _lib.stream(self.device)), "rework_collapse")

    def state_dict(self) -> dict:
        return dict(self.params)

    def load_state_dict(self, sd) -> None:
        """A CollectModelRework state_dict (the reference's parameter names); the shapes are checked by name, then the
        layers are collapsed again."""
        self._set(sd)

    @property
    def collapsed_weight(self) -> torch.Tensor:
        nq, D = self.n_rot + self.n_ph, self.n_features + 2
        return self.collapsed[: nq * D].view(nq, D)

    @property
    def collapsed_bias(self) -> torch.Tensor:
        nq, D = self.n_rot + self.n_ph, self.n_features + 2
        return self.collapsed[nq * D: nq * D + nq]

    def _rows(self, obs, agent_state, logits, env, out):
        """The checks act and act_select share -> (lead shape, rows, obs_format, rotation, pheromone): `out` = (rot, ph),
        int8 tensors of one element per row that receive the actions, else the policy's own reused buffers."""
        assert self.collapsed is not None, "ReworkPolicy on %s holds weights only: the kernel needs a GPU device" % self.device
        lead, m = check_rows(self.n_features, obs, agent_state, env)
        if logits is not None:
            assert logits.shape == (m, self.n_rot + self.n_ph) and logits.dtype == torch.float32 and logits.is_contiguous()
        if out is not None:
            rot, ph = out
            for t in (rot, ph):
                assert t.dtype == torch.int8 and t.numel() == m and t.is_contiguous() and t.device == obs.device
        else:
            if self._rot is None or self._rot.numel() != m:
                self._rot = torch.empty((m,), dtype=torch.int8, device=self.device)
                self._ph = torch.empty((m,), dtype=torch.int8, device=self.device)
            rot, ph = self._rot, self._ph
        fmt = 1 if obs.dtype == torch.bfloat16 else 0  # ANTSRL_OBS_BF16 / ANTSRL_OBS_F32
        return lead, m, fmt, rot, ph

    def act(self, obs: torch.Tensor, agent_state: torch.Tensor, logits: Optional[torch.Tensor] = None, env=None, out=None):
        """CollectAgentRework.get_action's network branch (:167-174): obs [..., P, P, K] float32 (or bfloat16 from a
        BatchedAntsEnv(obs_dtype=torch.bfloat16)) and agent_state float32 [..., 2] on the device ->
        (rotation int8 [...], pheromone int8 [...]), ready to pass to step().  `logits` (float32 [M, n_rot + n_ph])
        receives both heads' q.  The returned tensors are reused buffers, or views of `out` = (rot, ph) when the caller
        owns them."""
        lead, m, fmt, rot, ph = self._rows(obs, agent_state, logits, env, out)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_policy_rework(C.byref(self.shape), _p(self.collapsed), _p(obs), fmt, _p(agent_state),
                                                      m, _p(rot), _p(ph), _p(logits), _lib.stream(self.device)),
                       "policy_rework")
        return rot.view(lead), ph.view(lead)

    def act_select(self, obs: torch.Tensor, agent_state: torch.Tensor, *, seed: int, step: int, env_id_base: int, n_envs: int,
                   n_ants: int, epsilon: float, out=None, explored: Optional[torch.Tensor] = None,
                   logits: Optional[torch.Tensor] = None, env=None):
        """get_action with its epsilon branch (:165-174) in one launch (antsrl_policy_rework_select): act() on n_envs
        colonies of n_ants ants each, with the colonies that explore at (seed, step) taking the draw specification's
        uniform actions instead: the bits of act() followed by antsrl_agent_select_actions, without the forward pass of
        the rows that would be overwritten.  `explored` (uint8 [n_envs]) receives 1 for an exploring colony; `logits`
        is written for the rows of the other colonies only."""
        lead, m, fmt, rot, ph = self._rows(obs, agent_state, logits, env, out)
        assert m == n_envs * n_ants, "%d rows are not %d colonies of %d ants" % (m, n_envs, n_ants)
        if explored is not None:
            assert explored.dtype == torch.uint8 and explored.numel() == n_envs and explored.is_contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.antsrl_policy_rework_select(C.byref(self.shape), _p(self.collapsed), _p(obs), fmt,
                                                             _p(agent_state), seed, step, env_id_base, n_envs, n_ants,
                                                             float(epsilon), _p(rot), _p(ph), _p(explored), _p(logits),
                                                             _lib.stream(self.device)), "policy_rework_select")
        return rot.view(lead), ph.view(lead)
