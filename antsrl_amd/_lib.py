"""ctypes binding of libantsrl_hip.so (include/antsrl.h).  Fails loudly: there is no CPU
fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os

from .config import AntsCfg, AntsGen, AntsInit

LIB_PATH = os.environ.get("ANTSRL_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                        "libantsrl_hip.so")  # ANTSRL_LIB: A/B builds

#: every symbol include/antsrl.h declares
EXPORTS = ("antsrl_abi_version", "antsrl_cfg_size", "antsrl_last_error", "antsrl_workspace_bytes", "antsrl_create",
           "antsrl_workspace_bytes2", "antsrl_create2", "antsrl_workspace_map",
           "antsrl_destroy", "antsrl_reset", "antsrl_generate", "antsrl_step", "antsrl_observe", "antsrl_update", "antsrl_flush",
           "antsrl_step_update", "antsrl_set_timing_events", "antsrl_set_activation", "antsrl_policy_mlp", "antsrl_read_state", "antsrl_state_bytes",
           "antsrl_set_obs_format", "antsrl_query", "antsrl_bench_copy", "antsrl_set_inloop_policy", "antsrl_set_obs_row_stride", "antsrl_set_perceive_path", "antsrl_refresh_explored_summary", "antsrl_mem_alloc", "antsrl_mem_free",
           "antsrl_mem_trim", "antsrl_mem_stats", "antsrl_update_phase",
           "antsrl_perceptive_field", "antsrl_memnet_packed_bytes", "antsrl_memnet_pack", "antsrl_policy_memory",
           "antsrl_memtrain_sizes", "antsrl_memtrain_init", "antsrl_memtrain_unpack", "antsrl_memtrain_copy",
           "antsrl_memtrain_grad", "antsrl_memtrain_apply", "antsrl_memnet_packed_bytes_ex", "antsrl_memnet_pack_ex",
           "antsrl_policy_memory_ex", "antsrl_agent_select", "antsrl_replay_record_pre", "antsrl_replay_record_post",
           "antsrl_policy_memory_tiles", "antsrl_agent_plan", "antsrl_agent_select_actions",
           "antsrl_replay_record_pre_plain", "antsrl_replay_record_post_plain", "antsrl_lintrain_sizes",
           "antsrl_lintrain_grad", "antsrl_lintrain_apply", "antsrl_lintrain_step", "antsrl_exptrain_sizes",
           "antsrl_exptrain_grad", "antsrl_exptrain_apply", "antsrl_exptrain_step", "antsrl_rework_collapsed_bytes",
           "antsrl_rework_collapse", "antsrl_policy_rework", "antsrl_reworktrain_sizes", "antsrl_reworktrain_grad",
           "antsrl_reworktrain_apply", "antsrl_reworktrain_step", "antsrl_policy_rework_select", "antsrl_monitor_sizes",
           "antsrl_monitor_init", "antsrl_monitor_step", "antsrl_monitor_end_episode", "antsrl_recorder_sizes",
           "antsrl_recorder_begin", "antsrl_recorder_frame", "antsrl_render_sizes", "antsrl_render_frames",
           "antsrl_stats_sizes", "antsrl_stats_row", "antsrl_jointtrain_sizes", "antsrl_jointtrain_grad",
           "antsrl_jointtrain_apply", "antsrl_jointtrain_step", "antsrl_obs_coords", "antsrl_give_reward",
           "antsrl_checkpoint_map", "antsrl_checkpoint_save", "antsrl_checkpoint_load", "antsrl_fork_envs",
           "antsrl_pop_policy", "antsrl_pop_select", "antsrl_pop_record_pre", "antsrl_pop_record_post",
           "antsrl_pop_lintrain_step", "antsrl_pop_explore_policy", "antsrl_pop_exptrain_sizes",
           "antsrl_pop_exptrain_step", "antsrl_pop_joint_policy", "antsrl_pop_jointtrain_sizes",
           "antsrl_pop_jointtrain_step", "antsrl_pop_memtrain_sizes", "antsrl_pop_memtrain_step",
           "antsrl_pop_memnet_sizes", "antsrl_pop_policy_memory", "antsrl_pop_memory_select",
           "antsrl_pop_memory_record_pre", "antsrl_pop_memory_record_post", "antsrl_pop_rework_collapse",
           "antsrl_pop_policy_rework", "antsrl_pop_policy_rework_select", "antsrl_pop_reworktrain_sizes",
           "antsrl_pop_reworktrain_step", "antsrl_pop_fitness", "antsrl_pop_exploit")

_lib = None


class AntsMemNetShape(C.Structure):
    """include/antsrl.h AntsMemNetShape."""
    _fields_ = [(n, C.c_int32) for n in ("n_features", "agent_dim", "mem_size", "h1", "h2", "h3", "n_rot", "n_ph")]


class AntsReworkShape(C.Structure):
    """include/antsrl.h AntsReworkShape."""
    _fields_ = [(n, C.c_int32) for n in ("n_features", "agent_dim", "g1", "g2", "g3", "r1", "r2", "r3", "p1", "n_rot", "n_ph")]


class AntsRecordSpec(C.Structure):
    """include/antsrl.h AntsRecordSpec."""
    _fields_ = [(n, C.c_int32) for n in ("n_envs", "n_ants", "env_id_base", "n_features", "agent_dim", "mem_size", "n_rot",
                                         "obs_format", "obs_pitch", "reserved")] + [
        (n, C.c_int64) for n in ("K", "head", "max_len")] + [(n, C.c_uint64) for n in ("seed", "step")]


class AntsRenderOpts(C.Structure):
    """include/antsrl.h AntsRenderOpts."""
    _fields_ = [(n, C.c_int32) for n in ("zoom", "view_mask", "ant_radius", "layer_only")] + [
        ("phero_max_val", C.c_double), ("phero_colors", (C.c_uint8 * 3) * 4)]


class AntsWsArray(C.Structure):
    """include/antsrl.h AntsWsArray."""
    _fields_ = [("name", C.c_char * 24), ("block", C.c_int32), ("_pad", C.c_int32), ("offset", C.c_uint64), ("bytes", C.c_uint64)]


class AntsCkptArray(C.Structure):
    """include/antsrl.h AntsCkptArray."""
    _fields_ = [("name", C.c_char * 24), ("offset", C.c_uint64), ("bytes_per_env", C.c_uint64)]


POP_MAX = 64  # include/antsrl.h ANTSRL_POP_MAX


class AntsPopMember(C.Structure):
    """include/antsrl.h AntsPopMember."""
    _fields_ = [("seed", C.c_uint64), ("epsilon", C.c_double), ("learning_rate", C.c_double), ("discount", C.c_float),
                ("reserved", C.c_int32)]


class AntsPopSpec(C.Structure):
    """include/antsrl.h AntsPopSpec."""
    _fields_ = [(n, C.c_int32) for n in ("n_members", "n_envs", "n_ants", "env_id_base", "n_features", "obs_format",
                                         "obs_pitch", "reserved")] + [("members", AntsPopMember * POP_MAX)]


class AntsrlError(RuntimeError):
    pass


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AntsrlError(
            "libantsrl_hip.so is missing (%s): build it with `python -m antsrl_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 (same sonames as /opt/rocm).
    # A process must hold ONE HIP runtime: import torch first so the NEEDED entries of
    # libantsrl_hip.so bind to the runtime torch's streams and tensors live in.  (Loaded the
    # other way round, launches fail with "no ROCm-capable device is detected".)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    lib.antsrl_abi_version.restype = i32
    lib.antsrl_last_error.restype = C.c_char_p
    lib.antsrl_workspace_bytes.argtypes = [C.POINTER(AntsCfg), C.POINTER(C.c_size_t)]
    lib.antsrl_create.argtypes = [C.POINTER(AntsCfg), vp, C.c_size_t, C.POINTER(vp)]
    lib.antsrl_workspace_bytes2.argtypes = [C.POINTER(AntsCfg), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.antsrl_create2.argtypes = [C.POINTER(AntsCfg), vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp)]
    lib.antsrl_workspace_map.argtypes = [C.POINTER(AntsCfg), i32, C.POINTER(AntsWsArray), C.c_int32, C.POINTER(C.c_int32)]
    lib.antsrl_destroy.argtypes = [vp]
    lib.antsrl_destroy.restype = None
    lib.antsrl_reset.argtypes = [vp, C.POINTER(AntsInit), vp]
    lib.antsrl_generate.argtypes = [vp, C.POINTER(AntsGen), C.c_uint64, vp]
    lib.antsrl_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.antsrl_observe.argtypes = [vp, vp, vp, vp, vp]
    lib.antsrl_update.argtypes = [vp, vp, vp]
    lib.antsrl_flush.argtypes = [vp, vp]
    lib.antsrl_checkpoint_map.argtypes = [C.POINTER(AntsCfg), C.POINTER(AntsCkptArray), C.c_int32, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.antsrl_checkpoint_save.argtypes = [vp, vp, vp, vp]
    lib.antsrl_checkpoint_load.argtypes = [vp, vp, vp, vp]
    lib.antsrl_fork_envs.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, vp]
    lib.antsrl_update_phase.argtypes = [vp, i32, vp, vp]
    lib.antsrl_perceptive_field.argtypes = [vp, vp, vp]
    lib.antsrl_obs_coords.argtypes = [vp, vp, vp]
    lib.antsrl_give_reward.argtypes = [vp, vp, C.c_double, vp, vp]
    lib.antsrl_step_update.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.antsrl_set_timing_events.argtypes = [vp, C.POINTER(vp)]
    lib.antsrl_set_activation.argtypes = [vp, vp, C.c_double, vp]
    lib.antsrl_policy_mlp.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.antsrl_read_state.argtypes = [vp, i32, vp, vp]
    lib.antsrl_state_bytes.argtypes = [vp, i32, C.POINTER(C.c_size_t)]
    lib.antsrl_set_obs_format.argtypes = [vp, i32]
    lib.antsrl_query.argtypes = [vp, i32, C.POINTER(C.c_longlong)]
    lib.antsrl_set_inloop_policy.argtypes = [vp, i32] + [vp] * 9
    lib.antsrl_bench_copy.argtypes = [vp, vp, C.c_size_t, vp]
    lib.antsrl_set_obs_row_stride.argtypes = [vp, i32]
    lib.antsrl_set_perceive_path.argtypes = [vp, i32]
    lib.antsrl_refresh_explored_summary.argtypes = [vp, vp]
    lib.antsrl_mem_alloc.argtypes = [C.c_size_t, i32, C.POINTER(vp)]
    lib.antsrl_mem_free.argtypes = [vp]
    lib.antsrl_mem_trim.argtypes = []
    lib.antsrl_mem_stats.argtypes = [C.POINTER(C.c_size_t)] * 4
    lib.antsrl_memnet_packed_bytes.argtypes = [C.POINTER(AntsMemNetShape), C.POINTER(C.c_size_t)]
    lib.antsrl_memnet_pack.argtypes = [C.POINTER(AntsMemNetShape), C.POINTER(vp), vp, vp]
    lib.antsrl_policy_memory.argtypes = [C.POINTER(AntsMemNetShape), vp, vp, i32, vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.antsrl_memnet_packed_bytes_ex.argtypes = [C.POINTER(AntsMemNetShape), i32, C.POINTER(C.c_size_t)]
    lib.antsrl_memnet_pack_ex.argtypes = [C.POINTER(AntsMemNetShape), i32, C.POINTER(vp), vp, vp]
    lib.antsrl_policy_memory_ex.argtypes = [C.POINTER(AntsMemNetShape), i32, vp, vp, i32, vp, vp, C.c_int64, vp, vp, vp,
                                            vp, vp]
    lib.antsrl_policy_memory_tiles.argtypes = [C.POINTER(AntsMemNetShape), i32, vp, vp, i32, vp, vp, C.c_int64, vp, vp, vp,
                                               vp, vp, vp, vp]
    sz = C.POINTER(C.c_size_t)
    lib.antsrl_memtrain_sizes.argtypes = [C.POINTER(AntsMemNetShape), C.c_int64, sz, sz, sz, sz]
    lib.antsrl_memtrain_init.argtypes = [C.POINTER(AntsMemNetShape), C.POINTER(vp), vp, vp]
    lib.antsrl_memtrain_unpack.argtypes = [C.POINTER(AntsMemNetShape), vp, C.POINTER(vp), vp]
    lib.antsrl_memtrain_copy.argtypes = [C.POINTER(AntsMemNetShape), vp, vp, vp]
    lib.antsrl_memtrain_grad.argtypes = [C.POINTER(AntsMemNetShape), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64,
                                         C.c_float, vp, vp, vp, vp]
    lib.antsrl_memtrain_apply.argtypes = [C.POINTER(AntsMemNetShape), vp, vp, C.c_int64, C.c_double, C.c_double,
                                          C.c_double, C.c_double, vp]
    lib.antsrl_agent_select.argtypes = [C.c_uint64, C.c_uint64, i32, i32, i32, C.c_double, i32, i32, i32, vp, vp, vp, vp,
                                        vp, vp]
    lib.antsrl_agent_plan.argtypes = [C.c_uint64, C.c_uint64, i32, i32, i32, C.c_double, vp, vp, vp]
    lib.antsrl_replay_record_pre.argtypes = [C.POINTER(AntsRecordSpec)] + [vp] * 9
    lib.antsrl_replay_record_post.argtypes = [C.POINTER(AntsRecordSpec)] + [vp] * 10
    lib.antsrl_agent_select_actions.argtypes = [C.c_uint64, C.c_uint64, i32, i32, i32, C.c_double, i32, i32, vp, vp, vp, vp]
    lib.antsrl_replay_record_pre_plain.argtypes = [C.POINTER(AntsRecordSpec)] + [vp] * 8
    lib.antsrl_replay_record_post_plain.argtypes = [C.POINTER(AntsRecordSpec)] + [vp] * 9
    lib.antsrl_rework_collapsed_bytes.argtypes = [C.POINTER(AntsReworkShape), sz]
    lib.antsrl_rework_collapse.argtypes = [C.POINTER(AntsReworkShape), C.POINTER(vp), vp, vp]
    lib.antsrl_policy_rework.argtypes = [C.POINTER(AntsReworkShape), vp, vp, i32, vp, C.c_int64, vp, vp, vp, vp]
    rs = C.POINTER(AntsReworkShape)
    lib.antsrl_policy_rework_select.argtypes = [rs, vp, vp, i32, vp, C.c_uint64, C.c_uint64, i32, i32, i32, C.c_double, vp, vp,
                                                vp, vp, vp]
    # the four flat trainers (antsrl_<entry>_sizes / _grad / _apply / _step): one argument order behind the net's own
    # leading arguments.  entry: (what _grad and _step take in front of the arrays, what _apply takes in front of Adam's m)
    adam = [C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double]            # step, lr, beta1, beta2, eps
    arrays = [vp] * 7 + [C.c_int64, vp, C.c_int64, C.c_float]                     # the seven arrays, n_rows, idx, B, discount
    for entry, (net, apply_net) in {"lintrain": ([i32] + [vp] * 4, [vp]), "exptrain": ([i32, vp, vp], [i32, vp]),
                                    "jointtrain": ([i32, vp, vp], [i32, vp]), "reworktrain": ([rs, vp, vp], [rs, vp])}.items():
        for stage, argtypes in (("sizes", [net[0], C.c_int64, sz, sz, C.POINTER(C.c_int32)]),
                                ("grad", net + arrays + [vp, vp, vp, vp]),                  # grads, loss, workspace, stream
                                ("apply", apply_net + [vp, vp, vp] + adam + [vp]),          # adam_m, adam_v, grads; stream
                                ("step", net + [vp, vp] + arrays + adam + [vp, vp, vp, vp])):  # adam_m, adam_v behind the net
            getattr(lib, "antsrl_%s_%s" % (entry, stage)).argtypes = argtypes
    lib.antsrl_monitor_sizes.argtypes = [i32, i32, i32, i32, sz]
    lib.antsrl_monitor_init.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.antsrl_monitor_step.argtypes = [vp, i32, i32, i32, i32, vp, vp, C.c_double, i32, i32, vp]
    lib.antsrl_monitor_end_episode.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp]
    lib.antsrl_recorder_sizes.argtypes = [vp, i32, i32, i32, sz, sz, sz]
    lib.antsrl_recorder_begin.argtypes = [vp, vp, C.POINTER(C.c_int32), i32, i32, i32, vp]
    lib.antsrl_recorder_frame.argtypes = [vp, vp, C.POINTER(C.c_int32), i32, i32, i32, i32, vp]
    lib.antsrl_render_sizes.argtypes = [vp, i32, C.POINTER(AntsRenderOpts), sz, sz]
    lib.antsrl_render_frames.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.POINTER(AntsRenderOpts), vp, vp, vp]
    lib.antsrl_stats_sizes.argtypes = [vp, i32, sz, sz, sz]
    lib.antsrl_stats_row.argtypes = [vp, vp, i32, i32, vp]
    ps = C.POINTER(AntsPopSpec)
    lib.antsrl_pop_policy.argtypes = [ps] + [vp] * 9
    lib.antsrl_pop_select.argtypes = [ps, C.c_uint64, vp, vp, vp, vp]
    lib.antsrl_pop_record_pre.argtypes = [ps, C.c_uint64, C.c_int64, C.c_int64, C.c_int64] + [vp] * 8
    lib.antsrl_pop_record_post.argtypes = [ps, C.c_uint64, C.c_int64, C.c_int64, C.c_int64] + [vp] * 9
    lib.antsrl_pop_lintrain_step.argtypes = [ps] + [vp] * 12 + [C.c_int64, vp, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                                                C.c_double, vp, vp, vp, i32, vp]
    lib.antsrl_pop_explore_policy.argtypes = [ps] + [vp] * 5
    lib.antsrl_pop_exptrain_sizes.argtypes = [i32, C.c_int64, i32, sz, sz, sz, C.POINTER(C.c_int32)]
    lib.antsrl_pop_exptrain_step.argtypes = [ps] + [vp] * 11 + [C.c_int64, vp, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                                                C.c_double, vp, vp, vp, i32, vp, vp]
    lib.antsrl_pop_joint_policy.argtypes = [ps] + [vp] * 7
    lib.antsrl_pop_jointtrain_sizes.argtypes = lib.antsrl_pop_exptrain_sizes.argtypes
    lib.antsrl_pop_jointtrain_step.argtypes = lib.antsrl_pop_exptrain_step.argtypes
    lib.antsrl_pop_memtrain_sizes.argtypes = [C.POINTER(AntsMemNetShape), C.c_int64, i32, sz, sz, sz, sz, C.POINTER(C.c_int32)]
    lib.antsrl_pop_memtrain_step.argtypes = [ps, C.POINTER(AntsMemNetShape)] + lib.antsrl_pop_exptrain_step.argtypes[3:]
    ms = C.POINTER(AntsMemNetShape)
    lib.antsrl_pop_memnet_sizes.argtypes = [ms, i32, i32, sz, sz]
    lib.antsrl_pop_policy_memory.argtypes = [ps, ms, i32] + [vp] * 9
    lib.antsrl_pop_memory_select.argtypes = [ps, ms, C.c_uint64] + [vp] * 6
    # the record pair's arguments with the shape behind the spec and `memory` behind agent_state
    lib.antsrl_pop_memory_record_pre.argtypes = [ps, ms] + lib.antsrl_pop_record_pre.argtypes[1:] + [vp]
    lib.antsrl_pop_memory_record_post.argtypes = [ps, ms] + lib.antsrl_pop_record_post.argtypes[1:] + [vp]
    lib.antsrl_pop_rework_collapse.argtypes = [rs, i32, vp, vp, vp]
    lib.antsrl_pop_policy_rework.argtypes = [ps, rs] + [vp] * 7
    lib.antsrl_pop_policy_rework_select.argtypes = [ps, rs, vp, vp, vp, C.c_uint64] + [vp] * 5
    lib.antsrl_pop_reworktrain_sizes.argtypes = [rs, C.c_int64, i32, sz, sz, sz, sz, C.POINTER(C.c_int32)]
    lib.antsrl_pop_reworktrain_step.argtypes = [ps, rs] + lib.antsrl_pop_exptrain_step.argtypes[1:]
    lib.antsrl_pop_fitness.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.antsrl_pop_exploit.argtypes = [i32, C.POINTER(vp), C.POINTER(C.c_uint64), i32, i32, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), vp]
    for name in EXPORTS:
        getattr(lib, name)  # AttributeError if the build lost a symbol
    lib.antsrl_cfg_size.restype = C.c_size_t
    from .config import ABI_VERSION
    if lib.antsrl_abi_version() != ABI_VERSION:
        raise AntsrlError("ABI version mismatch: library %d, binding %d" % (lib.antsrl_abi_version(), ABI_VERSION))
    if lib.antsrl_cfg_size() != C.sizeof(AntsCfg):
        raise AntsrlError("AntsCfg layout mismatch: library %d bytes, binding %d" % (
            lib.antsrl_cfg_size(), C.sizeof(AntsCfg)))
    _lib = lib
    return lib


def hip_runtime() -> C.CDLL:
    """The libamdhip64 this process already uses (torch's), for raw hipEvent_t handling."""
    load()
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise AntsrlError("no libamdhip64 mapped in this process")


def check(rc: int, what: str = "antsrl") -> None:
    if rc != 0:
        msg = load().antsrl_last_error().decode("utf-8", "replace")
        raise AntsrlError("%s failed (%d): %s" % (what, rc, msg))


def ptr(t):
    """A tensor's device address for the ABI (None stays NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device):
    """The current torch stream of `device` as the ABI's `void *stream`."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class HipEvents:
    """Raw hipEvent_t handles (the ABI hook records them on the launch stream)."""

    def __init__(self, n):
        self.hip = hip_runtime()  # the runtime torch already loaded, not a second copy
        self.ev = []
        for _ in range(n):
            e = C.c_void_p()
            rc = self.hip.hipEventCreate(C.byref(e))
            assert rc == 0, "hipEventCreate failed: %d" % rc
            self.ev.append(e)

    def elapsed_ms(self, a, b):
        ms = C.c_float()
        rc = self.hip.hipEventElapsedTime(C.byref(ms), self.ev[a], self.ev[b])
        assert rc == 0, "hipEventElapsedTime failed: %d" % rc
        return ms.value

    def destroy(self):
        for e in self.ev:
            self.hip.hipEventDestroy(e)
