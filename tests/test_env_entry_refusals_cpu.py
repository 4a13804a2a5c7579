"""The environment's C entries on the host (include/antsrl.h): what each refuses before it touches the state, word for
word.  Every entry names its own NULL arguments ("NULL handle", "NULL handle or dst", ...); those that need an episode
refuse a handle that was never reset, and do so BEFORE they look at a selector or a phase; the setters and antsrl_query
refuse a selector they do not know.  The handles stand over a fake workspace pointer (as in
tests/test_colony_stats_abi_cpu.py) and every other pointer is a fake address, so a call that got as far as a launch would
not return ANTSRL_E_INVALID with the message asserted here.  No kernel is launched.

(The refusals while an Environment.update is in progress need a handle that has been reset, which takes a device:
tests/test_gpu_update_phases.py holds them.)"""
import ctypes as C

import pytest

from antsrl_amd import _lib
from antsrl_amd import build as buildmod
from antsrl_amd import config as cm

P = 1 << 20  # a fake, aligned device address
OBS_F32 = 0  # ANTSRL_OBS_F32 (include/antsrl.h)
NOT_RESET = b"antsrl_reset has not been called on this handle"

# entry -> (its NULL-handle words, the arguments behind the handle: fake and non-NULL throughout)
STATE_ENTRIES = {
    "antsrl_step": (b"NULL handle", (P, P, P, P, P, P, None)),
    "antsrl_observe": (b"NULL handle", (P, P, P, None)),
    "antsrl_update": (b"NULL handle", (P, None)),
    "antsrl_update_phase": (b"NULL handle", (cm.PHASE_WALLS, P, None)),
    "antsrl_step_update": (b"NULL handle", (P, P, P, P, P, P, P, None)),
    "antsrl_set_activation": (b"NULL handle or act", (P, 0.0, None)),
    "antsrl_refresh_explored_summary": (b"NULL handle", (None,)),
    "antsrl_read_state": (b"NULL handle or dst", (cm.S_PHERO, P, None)),
    "antsrl_perceptive_field": (b"NULL handle or dst", (P, None)),
}
# the entries that ask for no episode: setters, the query and the flush
OTHER_ENTRIES = {
    "antsrl_flush": (b"NULL handle", (None,)),
    "antsrl_query": (b"NULL handle or value", (cm.Q_TIMESTEP, C.pointer(C.c_longlong()))),
    "antsrl_set_obs_format": (b"NULL handle", (OBS_F32,)),
    "antsrl_set_obs_row_stride": (b"NULL handle", (0,)),
    "antsrl_set_perceive_path": (b"NULL handle", (cm.PERCEIVE_AUTO,)),
    "antsrl_set_inloop_policy": (b"NULL handle", (294, P, P, P, P, P, P, P, P, None)),
}


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


@pytest.fixture()
def h(lib):
    cfg = cm.make_cfg(3, 8, 16, 12)
    n = C.c_size_t()
    assert lib.antsrl_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
    h = C.c_void_p()
    assert lib.antsrl_create(C.byref(cfg), C.c_void_p(4096), n.value, C.byref(h)) == 0, lib.antsrl_last_error()
    yield h
    lib.antsrl_destroy(h)


def refused(lib, rc, message):
    assert rc == -1, (rc, lib.antsrl_last_error())  # ANTSRL_E_INVALID
    assert lib.antsrl_last_error() == message, (lib.antsrl_last_error(), message)


@pytest.mark.parametrize("name", list(STATE_ENTRIES) + list(OTHER_ENTRIES))
def test_a_null_handle_is_refused_in_the_entrys_own_words(lib, name):
    words, args = {**STATE_ENTRIES, **OTHER_ENTRIES}[name]
    refused(lib, getattr(lib, name)(None, *args), words)


@pytest.mark.parametrize("name", list(STATE_ENTRIES))
def test_a_handle_that_was_never_reset_is_refused(lib, h, name):
    refused(lib, getattr(lib, name)(h, *STATE_ENTRIES[name][1]), NOT_RESET)


def test_the_second_pointer_an_entry_names_is_refused_with_the_handle(lib, h):
    refused(lib, lib.antsrl_set_activation(h, None, 0.0, None), b"NULL handle or act")
    refused(lib, lib.antsrl_read_state(h, cm.S_PHERO, None, None), b"NULL handle or dst")
    refused(lib, lib.antsrl_perceptive_field(h, None, None), b"NULL handle or dst")
    refused(lib, lib.antsrl_query(h, cm.Q_TIMESTEP, None), b"NULL handle or value")


def test_the_unreset_refusal_comes_before_the_selector_and_the_phase(lib, h):
    for which in (-1, 999):
        refused(lib, lib.antsrl_read_state(h, which, P, None), NOT_RESET)
    for phase in (-1, 4, cm.PHASE_ANTS):
        refused(lib, lib.antsrl_update_phase(h, phase, P, None), NOT_RESET)
    # (and before the outputs antsrl_step / antsrl_step_update require)
    refused(lib, lib.antsrl_step(h, P, P, P, None, None, None, None), NOT_RESET)
    refused(lib, lib.antsrl_step_update(h, P, P, P, P, None, None, None, None), NOT_RESET)


def test_unknown_selectors_are_refused(lib, h):
    v = C.c_longlong(-7)
    for what in (-1, 9, 1 << 20):
        refused(lib, lib.antsrl_query(h, what, C.byref(v)), b"bad query selector %d" % what)
    assert v.value == -7
    for fmt in (-1, 2):
        refused(lib, lib.antsrl_set_obs_format(h, fmt), b"bad observation format %d" % fmt)
    for path in (-1, 3):
        refused(lib, lib.antsrl_set_perceive_path(h, path), b"bad perceive path %d" % path)


def test_what_asks_for_no_episode_works_on_a_fresh_handle(lib, h):
    v = C.c_longlong()
    assert lib.antsrl_query(h, cm.Q_TIMESTEP, C.byref(v)) == 0 and v.value == 1
    assert lib.antsrl_flush(h, None) == 0  # (nothing is deferred: no launch)
    assert lib.antsrl_set_obs_format(h, OBS_F32) == 0
    assert lib.antsrl_set_obs_row_stride(h, 0) == 0
    assert lib.antsrl_set_perceive_path(h, cm.PERCEIVE_GENERIC) == 0
    assert lib.antsrl_set_inloop_policy(h, 0, None, None, None, None, None, None, None, None, None) == 0  # (w1 NULL: off)
    refused(lib, lib.antsrl_step(h, P, P, P, P, P, P, None), NOT_RESET)  # (still no episode)
