"""antsrl_obs_coords and antsrl_give_reward on the host (include/antsrl.h, "A CALLER'S Reward"): both are declared, exported
and bound, the ABI version is still 5, and each refuses — in its own words, before anything is launched — a NULL
argument and a handle that was never reset.  The handles stand over a fake workspace pointer and every other pointer is a
fake address (as in tests/test_env_entry_refusals_cpu.py), so a call that got as far as a launch would not return
ANTSRL_E_INVALID with the message asserted here.

(The refusal between two phases of antsrl_update_phase and the deferred update they enqueue first need a handle that
has been reset, which takes a device: tests/test_gpu_custom_reward.py holds them.)"""
import ctypes as C
import os
import re

import pytest

from antsrl_amd import _lib
from antsrl_amd import build as buildmod
from antsrl_amd import config as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # a fake, aligned device address
NOT_RESET = b"antsrl_reset has not been called on this handle"
ENTRIES = ("antsrl_obs_coords", "antsrl_give_reward")


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


@pytest.fixture()
def h(lib):
    cfg = cm.make_cfg(3, 8, 16, 12, reward_kind=cm.REWARD_NONE, reward_threshold=float("inf"))  # (AntsCfg takes any double)
    n = C.c_size_t()
    assert lib.antsrl_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
    h = C.c_void_p()
    assert lib.antsrl_create(C.byref(cfg), C.c_void_p(4096), n.value, C.byref(h)) == 0, lib.antsrl_last_error()
    yield h
    lib.antsrl_destroy(h)


def refused(lib, rc, message):
    assert rc == -1, (rc, lib.antsrl_last_error())  # ANTSRL_E_INVALID
    assert lib.antsrl_last_error() == message, (lib.antsrl_last_error(), message)


def test_both_entries_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "antsrl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+antsrl_obs_coords\s*\(\s*AntsHandle\s*\*h,\s*int32_t\s*\*dst,\s*void\s*\*stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+antsrl_give_reward\s*\(\s*AntsHandle\s*\*h,\s*const\s+double\s*\*reward,\s*double\s+threshold,"
                     r"\s*float\s*\*reward_out,\s*void\s*\*stream\s*\)\s*;", text)
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), "libantsrl_hip.so does not export %s" % name
    assert lib.antsrl_obs_coords.argtypes == [C.c_void_p] * 3
    assert lib.antsrl_give_reward.argtypes == [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]


def test_the_abi_version_is_still_5(lib):
    assert lib.antsrl_abi_version() == 5 == cm.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "antsrl.h")).read()
    assert re.search(r"#define\s+ANTSRL_ABI_VERSION\s+5\b", text)


def test_null_arguments_are_refused_in_the_entries_own_words(lib, h):
    refused(lib, lib.antsrl_obs_coords(None, P, None), b"NULL handle or dst")
    refused(lib, lib.antsrl_obs_coords(h, None, None), b"NULL handle or dst")
    refused(lib, lib.antsrl_give_reward(None, P, 0.0, P, None), b"NULL handle or reward")
    refused(lib, lib.antsrl_give_reward(h, None, 0.0, P, None), b"NULL handle or reward")
    refused(lib, lib.antsrl_give_reward(h, None, 0.0, None, None), b"NULL handle or reward")


def test_a_handle_that_was_never_reset_is_refused(lib, h):
    refused(lib, lib.antsrl_obs_coords(h, P, None), NOT_RESET)
    refused(lib, lib.antsrl_obs_coords(h, P + 4, None), NOT_RESET)  # (before the alignment of dst is looked at)
    refused(lib, lib.antsrl_give_reward(h, P, 0.0, P, None), NOT_RESET)
    refused(lib, lib.antsrl_give_reward(h, P, float("-inf"), None, None), NOT_RESET)  # (reward_out is optional)
