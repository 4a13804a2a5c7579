"""antsrl_checkpoint_map / _save / _load and antsrl_fork_envs on the host (include/antsrl.h, "CHECKPOINT"): the four entries
are declared, exported and bound, the ABI version is still 5; the device block's layout follows antsrl_workspace_map
whatever the split; and each handle entry refuses, in its own words and before anything is launched, a NULL handle, a
handle that was never reset, a bad fork index list and a blob that is not this library's or another AntsCfg's.

The handles stand over a fake workspace pointer and every other device pointer is a fake address (as in
tests/test_custom_reward_abi_cpu.py), so a call that got as far as a launch would not return ANTSRL_E_INVALID with the
message asserted here.  The index rules and the blob's checks come before the handle's state is looked at, so a handle that
was never reset serves for them; what needs an episode is in tests/test_gpu_checkpoint.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from antsrl_amd import _lib
from antsrl_amd import build as buildmod
from antsrl_amd import config as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20  # a fake, aligned device address
NOT_RESET = b"antsrl_reset has not been called on this handle"
ENTRIES = ("antsrl_checkpoint_map", "antsrl_checkpoint_save", "antsrl_checkpoint_load", "antsrl_fork_envs")
MAGIC, VERSION = 0x4b435441, 1


def _diffuse3():
    f3 = np.ones((3, 3)) * 0.02
    f3[1, 1] = 1 - 8 * 0.02
    return f3 * (1 - 0.001)


#: the carve's four kinds: interleaved records (c3's layout), separate scaled buffers (three pheromones), the ping-pong
#: pair behind a diffusing filter, the single-kernel path
CASES = {
    "interleaved": lambda: cm.make_cfg(5, 33, 64, 64, n_rocks=2, deposit_strength=256.0),
    "three_phero": lambda: cm.make_cfg(5, 33, 64, 64, n_rocks=2, n_phero=3),
    "diffuse3x3": lambda: cm.make_cfg(5, 33, 64, 64, n_rocks=2, filt=_diffuse3()),
    "single_kernel": lambda: cm.make_cfg(5, 33, 64, 64, n_rocks=2, act_path=cm.ACT_SINGLE_KERNEL),
}
#: the record arrays each case must show (so that the four cases do cover four carves)
RECORDS = {"interleaved": {"records"}, "three_phero": {"phero0", "food"}, "diffuse3x3": {"phero0", "phero1", "food"},
           "single_kernel": {"records"}}


@pytest.fixture(scope="module")
def lib():
    buildmod.build_hip()
    return _lib.load()


@pytest.fixture()
def cfg():
    return cm.make_cfg(3, 8, 16, 12, n_rocks=1)


@pytest.fixture()
def h(lib, cfg):
    n = C.c_size_t()
    assert lib.antsrl_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
    h = C.c_void_p()
    assert lib.antsrl_create(C.byref(cfg), C.c_void_p(4096), n.value, C.byref(h)) == 0, lib.antsrl_last_error()
    yield h
    lib.antsrl_destroy(h)


def refused(lib, rc, message):
    assert rc == -1, (rc, lib.antsrl_last_error())  # ANTSRL_E_INVALID
    err = lib.antsrl_last_error()
    assert (err == message) if isinstance(message, bytes) else message.search(err), (err, message)


def _ws_map(lib, cfg, split):
    n = C.c_int32()
    assert lib.antsrl_workspace_map(C.byref(cfg), split, None, 0, C.byref(n)) == 0
    arr = (_lib.AntsWsArray * n.value)()
    assert lib.antsrl_workspace_map(C.byref(cfg), split, arr, n.value, C.byref(n)) == 0
    return [(a.name.decode(), a.bytes) for a in arr]


def _ck_map(lib, cfg):
    n, dev, host = C.c_int32(), C.c_size_t(), C.c_size_t()
    assert lib.antsrl_checkpoint_map(C.byref(cfg), None, 0, C.byref(n), C.byref(dev), C.byref(host)) == 0
    arr = (_lib.AntsCkptArray * n.value)()
    m = C.c_int32()
    assert lib.antsrl_checkpoint_map(C.byref(cfg), arr, n.value, C.byref(m), None, None) == 0 and m.value == n.value
    return [(a.name.decode(), a.offset, a.bytes_per_env) for a in arr], dev.value, host.value


def _blob(lib, cfg, magic=MAGIC, version=VERSION, size=None):
    """A blob as antsrl_checkpoint_save lays it out: magic, version, size, the AntsCfg, then the handle's fields (zeros)."""
    host = _ck_map(lib, cfg)[2]
    head = struct.pack("<IIQ", magic, version, host if size is None else size) + bytes(cfg)
    return head + bytes(host - len(head))


def test_the_entries_are_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "antsrl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef\s+struct\s+AntsCkptArray\s*\{\s*char\s+name\[24\];\s*uint64_t\s+offset,\s*bytes_per_env;\s*\}\s*AntsCkptArray;", text)
    assert re.search(r"\bint\s+antsrl_checkpoint_map\s*\(\s*const\s+AntsCfg\s*\*cfg,\s*AntsCkptArray\s*\*entries,\s*int32_t\s+cap,"
                     r"\s*int32_t\s*\*count,\s*size_t\s*\*device_bytes,\s*size_t\s*\*host_bytes\s*\)\s*;", text)
    assert re.search(r"\bint\s+antsrl_checkpoint_save\s*\(\s*AntsHandle\s*\*h,\s*void\s*\*device_block,\s*void\s*\*host_blob,"
                     r"\s*void\s*\*stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+antsrl_checkpoint_load\s*\(\s*AntsHandle\s*\*h,\s*const\s+void\s*\*device_block,"
                     r"\s*const\s+void\s*\*host_blob,\s*void\s*\*stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+antsrl_fork_envs\s*\(\s*AntsHandle\s*\*h,\s*const\s+int32_t\s*\*src,\s*const\s+int32_t\s*\*dst,"
                     r"\s*int32_t\s+n,\s*void\s*\*stream\s*\)\s*;", text)
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), "libantsrl_hip.so does not export %s" % name
    vp = C.c_void_p
    assert lib.antsrl_checkpoint_save.argtypes == [vp] * 4 and lib.antsrl_checkpoint_load.argtypes == [vp] * 4
    assert lib.antsrl_fork_envs.argtypes == [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, vp]
    assert C.sizeof(_lib.AntsCkptArray) == 40


def test_the_abi_version_is_still_5(lib):
    assert lib.antsrl_abi_version() == 5 == cm.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "antsrl.h")).read()
    assert re.search(r"#define\s+ANTSRL_ABI_VERSION\s+5\b", text)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_block_follows_the_workspace_map_whatever_the_split(lib, name):
    cfg = CASES[name]()
    E = cfg.n_envs
    entries, dev, host = _ck_map(lib, cfg)
    assert host >= 16 + C.sizeof(cm.AntsCfg)
    for split in (0, 1):
        ws = [(n, b) for n, b in _ws_map(lib, cfg, split) if n != "pol_pack"]
        assert [n for n, _ in ws] == [n for n, _, _ in entries]  # the carve's names, in its order, minus pol_pack
        off = 0
        for (wname, wbytes), (_, offset, bpe) in zip(ws, entries):
            assert bpe * E == wbytes, (wname, bpe, E, wbytes)  # environment-major, stored whole
            assert offset % 256 == 0 and offset == off, (wname, offset, off)  # 256-aligned and dense
            off = (off + wbytes + 255) // 256 * 256
        assert dev == off  # the end of the last array
    assert RECORDS[name] == {n for n, _, _ in entries} & {"records", "phero0", "phero1", "food"}
    assert "pol_pack" in [n for n, _ in _ws_map(lib, cfg, 0)]


def test_checkpoint_map_validates_its_arguments(lib, cfg):
    n = C.c_int32()
    bad = cfg.copy()
    bad.n_phero = 9
    assert lib.antsrl_checkpoint_map(C.byref(bad), None, 0, C.byref(n), None, None) == -1
    assert b"n_phero" in lib.antsrl_last_error()
    refused(lib, lib.antsrl_checkpoint_map(C.byref(cfg), None, 4, C.byref(n), None, None), b"checkpoint_map: entries is NULL or cap < 0")
    two = (_lib.AntsCkptArray * 2)()  # a short buffer takes the first entries, count reports them all
    assert lib.antsrl_checkpoint_map(C.byref(cfg), two, 2, C.byref(n), None, None) == 0
    assert n.value > 2 and [a.name for a in two] == [b"x", b"y"]


def test_a_null_handle_or_pointer_is_refused(lib, h, cfg):
    blob = _blob(lib, cfg)
    for args in ((None, P, blob), (h, None, blob), (h, P, None)):
        refused(lib, lib.antsrl_checkpoint_save(*args, None), b"checkpoint_save: NULL handle, device_block or host_blob")
        refused(lib, lib.antsrl_checkpoint_load(*args, None), b"checkpoint_load: NULL handle, device_block or host_blob")
    one = (C.c_int32 * 1)(0)
    for args in ((None, one, one), (h, None, one), (h, one, None)):
        refused(lib, lib.antsrl_fork_envs(*args, 1, None), b"fork_envs: NULL handle, src or dst")


def test_a_handle_that_was_never_reset_is_refused(lib, h, cfg):
    out = C.create_string_buffer(_ck_map(lib, cfg)[2])
    refused(lib, lib.antsrl_checkpoint_save(h, P, out, None), NOT_RESET)
    assert out.raw == bytes(len(out.raw))  # nothing was written
    refused(lib, lib.antsrl_checkpoint_load(h, P, _blob(lib, cfg), None), NOT_RESET)  # (a blob that passes every check)
    src, dst = (C.c_int32 * 2)(1, 1), (C.c_int32 * 2)(0, 2)
    refused(lib, lib.antsrl_fork_envs(h, src, dst, 2, None), NOT_RESET)  # (an index list that passes every check)


@pytest.mark.parametrize("src,dst,n,message", [
    ([1], [0], 0, b"fork_envs: n must be >= 1, got 0"),
    ([1], [0], -3, b"fork_envs: n must be >= 1, got -3"),
    ([-1], [0], 1, b"fork_envs: src[0] = -1 is not in [0, 3)"),
    ([1, 3], [0, 2], 2, b"fork_envs: src[1] = 3 is not in [0, 3)"),
    ([1], [-2], 1, b"fork_envs: dst[0] = -2 is not in [0, 3)"),
    ([1], [3], 1, b"fork_envs: dst[0] = 3 is not in [0, 3)"),
    ([1, 1], [0, 0], 2, b"fork_envs: dst 0 appears twice (dst[1])"),
    ([1, 0], [0, 2], 2, b"fork_envs: environment 0 is a src (src[1]) and a dst"),
    ([1], [1], 1, b"fork_envs: environment 1 is a src (src[0]) and a dst"),
], ids=["n0", "n_negative", "src_negative", "src_out_of_range", "dst_negative", "dst_out_of_range", "dst_twice",
        "dst_in_src", "onto_itself"])
def test_fork_index_rules(lib, h, src, dst, n, message):
    """E = 3.  Checked on the host before the handle's state is looked at (a handle that was never reset serves)."""
    s, d = (C.c_int32 * len(src))(*src), (C.c_int32 * len(dst))(*dst)
    refused(lib, lib.antsrl_fork_envs(h, s, d, n, None), message)


def test_a_foreign_blob_is_refused_with_the_field_named(lib, h, cfg):
    host = _ck_map(lib, cfg)[2]
    refused(lib, lib.antsrl_checkpoint_load(h, P, _blob(lib, cfg, magic=MAGIC + 1), None),
            b"checkpoint_load: host_blob has magic 0x4b435442, not 0x4b435441")
    refused(lib, lib.antsrl_checkpoint_load(h, P, _blob(lib, cfg, version=2), None),
            b"checkpoint_load: host_blob has format version 2, this library reads 1")
    refused(lib, lib.antsrl_checkpoint_load(h, P, _blob(lib, cfg, size=host - 8), None),
            b"checkpoint_load: host_blob says size %d, the format's is %d" % (host - 8, host))
    changes = dict(n_ants=9, max_time=77, delta=1.2, rng_seed=5, env_id_base=1, reward_threshold=2.0, fct_food=3.0,
                   phero_mode=cm.PHERO_EXPLICIT_SWEEP)
    for field, value in changes.items():
        other = cfg.copy()
        setattr(other, field, value)
        refused(lib, lib.antsrl_checkpoint_load(h, P, _blob(lib, other), None),
                re.compile(rb"^checkpoint_load: the checkpoint's AntsCfg differs from this handle's in %s \(byte \d+\)$" % field.encode()))
    other = cfg.copy()
    other.filter[0] = 0.5  # an array's element is named by its array
    other.mask[3] = 1 - other.mask[3]
    refused(lib, lib.antsrl_checkpoint_load(h, P, _blob(lib, other), None),
            re.compile(rb"AntsCfg differs from this handle's in mask \(byte \d+\)$"))  # the FIRST differing field
