"""Builds libantsrl_hip.so (hand-written HIP, gfx950 only) in-tree with hipcc.

    python -m antsrl_amd.build          # or antsrl_amd.build.build_hip()

-ffp-contract=off: the reference (numpy) rounds every product before adding; fused
multiply-add would change ant coordinates in the last bit.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libantsrl_hip.so")
SOURCES = ["antsrl_act.hip", "antsrl_perceive.hip", "antsrl_update.hip", "antsrl_sweep.hip", "antsrl_state.hip",
           "antsrl_capi.hip", "antsrl_policy.hip", "antsrl_mem.hip",
           "antsrl_memnet.hip", "antsrl_memnet_f32.hip", "antsrl_memtrain.hip", "antsrl_memagent.hip",
           "antsrl_memapi.hip", "antsrl_loopapi.hip", "antsrl_lintrain.hip", "antsrl_exptrain.hip", "antsrl_jointtrain.hip",
           "antsrl_linapi.hip",
           "antsrl_rework.hip", "antsrl_reworktrain.hip", "antsrl_reworkapi.hip", "antsrl_monitor.hip", "antsrl_recorder.hip",
           "antsrl_render.hip", "antsrl_stats.hip", "antsrl_logapi.hip", "antsrl_checkpoint.hip",
           "antsrl_population.hip", "antsrl_popexplore.hip", "antsrl_popjoint.hip", "antsrl_popmemtrain.hip",
           "antsrl_popmemnet.hip", "antsrl_poprework.hip", "antsrl_popfitness.hip", "antsrl_popapi.hip"]
HEADERS = [os.path.join(CSRC, h) for h in ("antsrl_device.h", "antsrl_util.h", "antsrl_update_env.h",
                                           "antsrl_update_one.h", "antsrl_flush.h", "antsrl_layout.h",
                                           "antsrl_lds_optin.h", "antsrl_fail.h", "antsrl_memnet.h",
                                           "antsrl_memnet_dev.h", "antsrl_memnet_bf16_dev.h", "antsrl_memnet_body.inc",
                                           "antsrl_agent_select_memory.inc", "antsrl_memtrain.h", "antsrl_memagent.h", "antsrl_loopapi.h",
                                           "antsrl_draw.h",
                                           "antsrl_adam.h", "antsrl_dqn.h", "antsrl_dqn_dev.h", "antsrl_lintrain.h",
                                           "antsrl_l1train.h", "antsrl_l1train_dev.h", "antsrl_exptrain.h", "antsrl_jointtrain.h", "antsrl_rework.h", "antsrl_reworktrain.h", "antsrl_monitor.h", "antsrl_monitor_dev.h",
                                           "antsrl_cellread.h", "antsrl_recorder.h", "antsrl_render.h", "antsrl_stats.h",
                                           "antsrl_launch.h", "antsrl_handle.h", "antsrl_checkpoint.h",
                                           "antsrl_policy_flat.h", "antsrl_memagent_dev.h", "antsrl_lintrain_dev.h",
                                           "antsrl_population.h", "antsrl_population_dev.h", "antsrl_policy_flat_body.inc",
                                           "antsrl_agent_select_actions.inc", "antsrl_replay_record_body.inc",
                                           "antsrl_lintrain_body.inc", "antsrl_exptrain_dev.h",
                                           "antsrl_exptrain_fwd_body.inc", "antsrl_jointtrain_dev.h",
                                           "antsrl_jointtrain_fwd_body.inc", "antsrl_memtrain_dev.h",
                                           "antsrl_memtrain_gemm_body.inc", "antsrl_memtrain_td_body.inc",
                                           "antsrl_memtrain_wgrad_body.inc", "antsrl_memtrain_finalize_body.inc",
                                           "antsrl_memtrain_adam_body.inc", "antsrl_reworkapi.h",
                                           "antsrl_rework_collapse_body.inc", "antsrl_rework_act_body.inc",
                                           "antsrl_reworktrain_down_body.inc", "antsrl_reworktrain_batch_body.inc",
                                           "antsrl_reworktrain_up_body.inc", "antsrl_reworktrain_grad_body.inc")] + [
    os.path.join(HERE, "..", "include", "antsrl.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17",
         "-Wall", "-Wno-unused-function"]


def hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (needs the ROCm toolchain)")


#: host-only translation units (no kernel in them): a change there moves no byte on the device
HOST_ONLY_SOURCES = ("antsrl_capi.hip", "antsrl_mem.hip", "antsrl_memapi.hip", "antsrl_loopapi.hip", "antsrl_linapi.hip",
                     "antsrl_reworkapi.hip", "antsrl_logapi.hip", "antsrl_popapi.hip")


def source_hash() -> str:
    """sha256 (first 16 hex digits) over the KERNEL sources (every translation unit with device code + the shared headers +
    the C-ABI header): what a measurement was taken ON (profiles/traffic_<config>.json records it; bench.py flags PMC
    figures that pre-date the kernels it runs)."""
    import hashlib
    h = hashlib.sha256()
    for path in sorted([os.path.join(CSRC, s) for s in SOURCES if s not in HOST_ONLY_SOURCES] + [os.path.normpath(x) for x in HEADERS]):
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def is_stale(path: str = LIB_PATH) -> bool:
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build_hip(force: bool = False, verbose: bool = False) -> str:
    """One hipcc process per source (they are independent translation units), then one link."""
    if not force and not is_stale():
        return LIB_PATH
    objdir = os.path.join(LIB_DIR, "obj_libantsrl_hip")
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in FLAGS if f != "-shared"]
    procs = []
    for src in SOURCES:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = [hipcc()] + flags + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((subprocess.Popen(cmd), obj, cmd))
    objs = []
    for pr, obj, cmd in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
        objs.append(obj)
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB_PATH])
    return LIB_PATH


if __name__ == "__main__":
    print(build_hip(force="--force" in sys.argv, verbose=True))
