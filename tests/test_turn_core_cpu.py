"""The coordinate arithmetic of ke_turn_luma without a GPU: csrc/ke_turn_core.h compiled with the host C++ compiler
(tests/_turn_core_cpu.cpp) into a temporary directory.

* The header's map, driven by host loops -- destination pixel by destination pixel, and tile by tile as the kernel walks --
  equals turned.turn(k, O.luma(picture)) for every k, on every shape 1..9 x 1..9 and on tile - 1, tile, tile + 1 and
  2 * tile + 3 in each dimension, for 1, 3 and 4 channels.  There is no tolerance: a permutation of bytes.
* The tiles' source rectangles cover every source pixel exactly once.
* The same source has a ``main`` that runs the sweep against a turn spelled out from the definition; it is built with
  AddressSanitizer and UBSan and run as a program of its own, every buffer exactly as large as its picture."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from kobato_eyes_amd import turned
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "_turn_core_cpu.cpp")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("turn_core_cpu") / "turn_core_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC, SOURCE, "-o", out])
    lib = C.CDLL(out)
    lib.tc_turn_luma.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.tc_turn_luma.restype = None
    lib.tc_turn_luma_tiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.tc_turn_luma_tiles.restype = C.c_int64
    lib.tc_dst_size.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.tc_dst_size.restype = None
    return lib


def sides(tile: int) -> list:
    return list(range(1, 10)) + [tile - 1, tile, tile + 1, 2 * tile + 3]


def test_the_tile_is_the_kernels(cpu):
    assert cpu.tc_tile() == 64                   # DESIGN section 4 and tests/test_gpu_turned_ssim.py's shapes are written for this value


def test_the_map_is_turn_k_and_the_tiles_cover_the_source_once(cpu):
    rng = np.random.default_rng(20261020)
    tile = cpu.tc_tile()
    cases = 0
    for w in sides(tile):
        for h in sides(tile):
            for ch in (1, 3, 4):
                px = rng.integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
                luma = O.luma(px)
                for k in range(8):
                    want = np.ascontiguousarray(turned.turn(k, luma))
                    dw, dh = C.c_int(), C.c_int()
                    cpu.tc_dst_size(k, w, h, C.byref(dw), C.byref(dh))
                    assert (dh.value, dw.value) == want.shape, (w, h, k)
                    gathered = np.full(want.shape, 0xAA, np.uint8)
                    cpu.tc_turn_luma(px.ctypes.data, w, h, ch, k, gathered.ctypes.data)
                    assert np.array_equal(gathered, want), (w, h, ch, k)
                    scattered, cover = np.full(want.shape, 0x55, np.uint8), np.zeros((h, w), np.int32)
                    faults = cpu.tc_turn_luma_tiles(px.ctypes.data, w, h, ch, k, scattered.ctypes.data, cover.ctypes.data)
                    assert faults == 0, (w, h, ch, k)
                    assert np.all(cover == 1), (w, h, ch, k)
                    assert np.array_equal(scattered, want), (w, h, ch, k)
                    cases += 1
    assert cases == 13 * 13 * 3 * 8


def test_sanitised_program(tmp_path):
    exe = str(tmp_path / "turn_core_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-DTURN_CORE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", CSRC, SOURCE, "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == f"ok {13 * 13 * 3 * 8}" and "runtime error" not in done.stderr
