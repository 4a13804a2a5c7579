"""The cell-record layout (antsrl_amd/csrc/antsrl_layout.h: blocks of 2 x 4 cells per 128-byte line, KP::tiled) checked on the host
with the SAME function the kernels use: g++ compiles the header and every cell of a list of grid shapes is enumerated — the
mapping is a bijection onto [0, W * H) and every block is one aligned run of eight records.  (The GPU suite then holds every
kernel that indexes the records to the oracle, with the blocks and — on grids they do not tile (odd W, H not a multiple
of 4: the fuzz cases) — without.)"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tiled_slot_is_a_bijection_with_aligned_blocks(tmp_path):
    so = str(tmp_path / "layout_check.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", os.path.join(HERE, "native", "layout_check.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.layout_violations.restype = C.c_long
    assert lib.layout_violations() == 0
