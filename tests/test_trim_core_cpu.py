"""The arithmetic of ke_content_boxes without a GPU: csrc/ke_trim_core.h compiled with the host C++ compiler
(tests/_trim_core_cpu.cpp) into a temporary directory and driven by host loops the way the kernel walks -- band by band, a
row per wave, a lane per aligned 16-byte vector.

* The walk equals the NumPy definition AND the issue's Pillow recipe on every shape 1..9 x 1..9, on widths whose rows cross
  the 16-byte vectors at every phase (5, 6, 21, 22, 43), on heights of band - 1, band, band + 1 and 2 * band + 3, for 1, 3
  and 4 channels, at every start alignment 0..15 and tolerances 0, 1, 48, 254 and 255 (no box).  No tolerance: integers.
* No vector but the first and the last of a picture reaches outside the picture's bytes.
* Single pixels: each corner and edge; one channel off by tol (no) and by tol + 1 (yes); the fourth byte alone (no box).
* The qualifying rule on a grid of (w, h, box) against its restatement.
* The same source has a ``main`` that runs the sweep against the definition spelled out in C++; it is built with
  AddressSanitizer and UBSan and run as a program of its own, every buffer ending exactly where its picture ends."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _trim_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "_trim_core_cpu.cpp")
BAND = 32      # KE_TRIM_BAND_ROWS: DESIGN section 4 and the seams of tests/test_gpu_trimmed.py are written for this value


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("trim_core_cpu") / "trim_core_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC, SOURCE, "-o", out])
    lib = C.CDLL(out)
    lib.tr_content_box.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.tr_content_box.restype = C.c_int64
    lib.tr_qualifies.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return lib


def walk(cpu, px: np.ndarray, tol: int, align: int = 0) -> tuple:
    """The kernel's walk over a copy of ``px`` that starts ``align`` bytes past a multiple of 16."""
    h, w = px.shape[:2]
    ch = 1 if px.ndim == 2 else px.shape[2]
    buf = np.zeros(px.size + 32, np.uint8)
    at = (align - buf.ctypes.data) % 16
    buf[at:at + px.size] = px.reshape(-1)
    box = np.full(4, -7, np.int32)
    faults = cpu.tr_content_box(buf.ctypes.data + at, w, h, ch, tol, box.ctypes.data)
    assert faults == 0, (w, h, ch, tol, align)
    return tuple(int(v) for v in box)


def test_the_band_is_the_kernels(cpu):
    assert cpu.tr_band_rows() == BAND


def test_the_walk_is_the_definition_and_the_pillow_recipe(cpu):
    rng = np.random.default_rng(T.SEED)
    cases = 0
    for w, h in T.grid_shapes(BAND):
        for ch in (1, 3, 4):
            px = T.grid_picture(rng, w, h, ch)
            for tol in T.TOLERANCES:
                want = T.content_box(px, tol)
                assert T.pillow_box(px, tol) == want, (w, h, ch, tol)
                if tol == 255:
                    assert want == (0, 0, 0, 0)
                for align in range(16):
                    assert walk(cpu, px, tol, align) == want, (w, h, ch, tol, align)
                    cases += 1
    assert cases == 12 * 13 * 3 * 5 * 16


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_single_pixels(cpu, ch):
    for tol in T.TOLERANCES:
        for name, px, want in T.single_pixel_cases(ch, tol):
            assert T.content_box(px, tol) == want, (name, tol)
            assert T.pillow_box(px, tol) == want, (name, tol)
            for align in (0, 1, 5, 15):
                assert walk(cpu, px, tol, align) == want, (name, ch, tol, align)


def test_a_uniform_picture_has_no_box(cpu):
    for ch in (1, 3, 4):
        px = np.full((40, 37, ch), 77, np.uint8)
        assert walk(cpu, px[:, :, 0] if ch == 1 else px, 0, 3) == (0, 0, 0, 0)


def test_the_qualifying_rule(cpu):
    from kobato_eyes_amd import trimmed

    cases = 0
    for w in (7, 8, 9, 49, 50, 51, 100, 400):
        for h in (7, 8, 9, 50, 101, 300):
            for bw in {0, 1, 7, 8, w - 8, w - 2, w - 1, w} - {-1}:
                for bh in {0, 1, 7, 8, h - 2, h - 1, h}:
                    if not (0 <= bw <= w and 0 <= bh <= h):
                        continue
                    for x0, y0 in ((0, 0), (w - bw, h - bh)):
                        box = np.array([x0, y0, x0 + bw, y0 + bh], np.int32)
                        want = T.qualifies(w, h, tuple(int(v) for v in box))
                        assert bool(cpu.tr_qualifies(w, h, box.ctypes.data)) == want, (w, h, box)
                        assert trimmed.qualifies(w, h, box) == want, (w, h, box)
                        cases += 1
    assert cases > 1000
    assert not T.qualifies(100, 100, (0, 0, 99, 99)) and T.qualifies(100, 100, (0, 0, 98, 100))      # one pixel is not 2 %
    assert not T.qualifies(100, 100, (0, 0, 7, 50)) and not T.qualifies(100, 100, (0, 0, 0, 0))


def test_sanitised_program(tmp_path):
    exe = str(tmp_path / "trim_core_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-DTRIM_CORE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", CSRC, SOURCE, "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == f"ok {12 * 13 * 3 * 16 * 5}" and "runtime error" not in done.stderr
