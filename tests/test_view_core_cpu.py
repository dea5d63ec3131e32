"""The coordinate arithmetic of ke_crop_turn_luma without a GPU: csrc/ke_view_core.h compiled with the host C++ compiler
(tests/_view_core_cpu.cpp) into a temporary directory.

* The header's map, driven by host loops -- destination pixel by destination pixel, and tile by tile as the kernel walks, rows
  read as the dwords the kernel reads with the image's pitch -- equals turned.turn(k, O.luma(picture)[y0:y1, x0:x1]) for every
  k, for box sides 1..9, tile - 1, tile, tile + 1 and 2 * tile + 3, every x0 and y0 in 0..3, images one to three pixels larger
  on the far sides, and 1, 3 and 4 channels.  There is no tolerance: a permutation of bytes.
* The tiles' source rectangles cover the box exactly once and touch no pixel outside it.
* The same source has a ``main`` that runs the sweep against a crop and a turn spelled out from the definition; it is built with
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
SOURCE = os.path.join(ROOT, "tests", "_view_core_cpu.cpp")
CASES = 13 * 13 * 4 * 4 * 3 * 8


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("view_core_cpu") / "view_core_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC, SOURCE, "-o", out])
    lib = C.CDLL(out)
    i = C.c_int
    lib.vc_view_luma.argtypes = [C.c_void_p, i, i, i, i, i, i, i, i, C.c_void_p]
    lib.vc_view_luma.restype = None
    lib.vc_view_luma_tiles.argtypes = [C.c_void_p, i, i, i, i, i, i, i, i, i, C.c_void_p, C.c_void_p]
    lib.vc_view_luma_tiles.restype = C.c_int64
    lib.vc_dst_size.argtypes = [i, i, i, C.c_void_p, C.c_void_p]
    lib.vc_dst_size.restype = None
    return lib


def sides(tile: int) -> list:
    return list(range(1, 10)) + [tile - 1, tile, tile + 1, 2 * tile + 3]


def test_the_tile_is_the_kernels(cpu):
    assert cpu.vc_tile() == 64 and sides(64)[-4:] == [63, 64, 65, 131]


def test_the_map_is_turn_k_of_the_crop_and_the_tiles_cover_the_box_once(cpu):
    rng = np.random.default_rng(20261020)
    tile = cpu.vc_tile()
    cases = 0
    for bw in sides(tile):
        for bh in sides(tile):
            for x0 in range(4):
                for y0 in range(4):
                    for ch in (1, 3, 4):
                        # one to three pixels of margin on the far sides, every count taken in turn
                        w, h = x0 + bw + 1 + cases // 8 % 3, y0 + bh + 1 + cases // 24 % 3
                        px = rng.integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
                        crop = O.luma(px)[y0:y0 + bh, x0:x0 + bw]
                        inside = np.zeros((h, w), np.int32)
                        inside[y0:y0 + bh, x0:x0 + bw] = 1
                        for k in range(8):
                            want = np.ascontiguousarray(turned.turn(k, crop))
                            dw, dh = C.c_int(), C.c_int()
                            cpu.vc_dst_size(k, bw, bh, C.byref(dw), C.byref(dh))
                            assert (dh.value, dw.value) == want.shape, (bw, bh, k)
                            at = (bw, bh, x0, y0, w, h, ch, k)
                            gathered = np.full(want.shape, 0xAA, np.uint8)
                            cpu.vc_view_luma(px.ctypes.data, w, h, ch, x0, y0, bw, bh, k, gathered.ctypes.data)
                            assert np.array_equal(gathered, want), at
                            scattered, cover = np.full(want.shape, 0x55, np.uint8), np.zeros((h, w), np.int32)
                            faults = cpu.vc_view_luma_tiles(px.ctypes.data, w, h, ch, x0, y0, bw, bh, k, cases % 4, scattered.ctypes.data,
                                                            cover.ctypes.data)
                            assert faults == 0, at
                            assert np.array_equal(cover, inside), at
                            assert np.array_equal(scattered, want), at
                            cases += 1
    assert cases == CASES


def test_sanitised_program(tmp_path):
    exe = str(tmp_path / "view_core_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-DVIEW_CORE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", CSRC, SOURCE, "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == f"ok {CASES}" and "runtime error" not in done.stderr
