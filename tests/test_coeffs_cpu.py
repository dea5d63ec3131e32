"""The resampler's tap tables without a GPU: csrc/ke_coeffs.cpp -- Pillow's taps, their three-byte-plane packing, the chunked
layout and the matrix-core operand layout -- compiled with the host C++ compiler into a stand-alone program
(tests/_coeffs_cpu.cpp), with AddressSanitizer and UBSan on, and run.

`check` holds every layout to the plain taps for the three filters on 18 (in, out) pairs, whole axes and fractional source
intervals (132 cases; the list is in the program).  `dump` prints the plain taps of one axis; this file applies them as
Pillow's two integer passes do -- per axis clip8((sum + 2^21) >> 22) to bytes, horizontal then vertical, an unchanged axis
skipped, very tall sources vertical first -- and compares with Image.resize byte for byte."""
from __future__ import annotations

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")

FILTERS = {0: Image.LANCZOS, 1: Image.BILINEAR, 2: Image.BICUBIC}       # include/keyes.h KE_FILTER_*
SHAPES = [(1, 1, 1, 7), (7, 1, 1, 1), (64, 64, 100, 90), (100, 64, 64, 100), (640, 37, 128, 37), (641, 40, 129, 17),
          (2340, 9, 130, 9), (40, 4096, 40, 16), (33, 257, 128, 129), (257, 31, 256, 33), (300, 200, 300, 77),
          (300, 200, 77, 200), (7, 1500, 5, 90)]
TALL_BOX = (7, 1500, 5, 90, (0.5, 10.25, 6.25, 1400.5))                   # a box on a source over 100 times taller than wide


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("coeffs") / "coeffs_cpu")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "_coeffs_cpu.cpp"),
                           os.path.join(CSRC, "ke_coeffs.cpp"), "-o", path])
    return path


def test_every_layout_rebuilds_the_plain_taps_under_the_sanitizers(exe):
    res = subprocess.run([exe, "check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    # 3 filters x (18 whole axes + 2 source intervals for each of the 13 pairs with in >= 20)
    assert res.stdout.strip().splitlines()[-1] == "ok cases=132", res.stdout[-2000:]


def _taps(exe, cache, in_size, out_size, filt, in0, in1):
    """(lo[out], cnt[out], kk[out][ksize]) of one axis from the program; the interval goes over in single precision, as
    Pillow's C entry point receives it."""
    key = (in_size, out_size, filt, float(np.float32(in0)), float(np.float32(in1)))
    if key not in cache:
        text = subprocess.check_output([exe, "dump", str(in_size), str(out_size), str(filt), "%.9g" % key[3], "%.9g" % key[4]], text=True)
        lines = text.strip().splitlines()
        ksize = int(lines[0].split()[1])
        assert len(lines) == out_size + 1
        lo, cnt, kk = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64), np.zeros((out_size, ksize), np.int64)
        for o, line in enumerate(lines[1:]):
            v = [int(x) for x in line.split()]
            lo[o], cnt[o] = v[0], v[1]
            assert len(v) == 2 + v[1] <= 2 + ksize
            kk[o, :v[1]] = v[2:]
        cache[key] = (lo, cnt, kk)
    return cache[key]


def _pass(img, axis, taps):
    """One of Pillow's integer passes along `axis` of a (h, w) byte image."""
    lo, cnt, kk = taps
    src = np.moveaxis(img.astype(np.int64), axis, -1)                     # (..., in)
    out = np.empty(src.shape[:-1] + (len(lo),), np.int64)
    for o in range(len(lo)):
        out[..., o] = src[..., lo[o]:lo[o] + cnt[o]] @ kk[o, :cnt[o]]
    out = np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def _resize_with_the_tables(exe, cache, img, ow, oh, filt, box):
    h, w = img.shape
    x0, y0, x1, y1 = box if box is not None else (0.0, 0.0, float(w), float(h))
    need_h = not (ow == w and x0 == 0 and x1 == w)
    need_v = not (oh == h and y0 == 0 and y1 == h)
    vertical_first = "self.size[1] > self.size[0] * 100 and size[1] < self.size[1]" in inspect.getsource(Image.Image.resize) \
        and h > w * 100 and oh < h
    # vertical first, Pillow resizes to (w, oh) with the box (0, y0, w, y1) and then to (ow, oh) with (x0, 0, x1, oh): the
    # same two single-axis passes in the other order
    steps = [(1, w, ow, x0, x1, need_h), (0, h, oh, y0, y1, need_v)]
    for axis, n_in, n_out, a, b, need in (steps[::-1] if vertical_first else steps):
        if need:
            img = _pass(img, axis, _taps(exe, cache, n_in, n_out, filt, a, b))
    return img


def _cases():
    for w, h, ow, oh in SHAPES:
        yield w, h, ow, oh, None
        if w > 20 and h > 20:
            yield w, h, ow, oh, (1.25, 2.5, w - 3.75, h - 0.5)
    yield TALL_BOX


@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_the_dumped_tables_applied_as_two_integer_passes_are_pillows_resize(exe, filt):
    cache, bad, n = {}, [], 0
    for k, (w, h, ow, oh, box) in enumerate(_cases()):
        img = np.random.default_rng(1000 + k).integers(0, 256, (h, w), dtype=np.uint8)
        if (w, h) == (ow, oh) and box is None:
            continue                                                      # Pillow copies; no table is involved
        want = np.asarray(Image.fromarray(img).resize((ow, oh), FILTERS[filt], box=box))
        got = _resize_with_the_tables(exe, cache, img, ow, oh, filt, box)
        n += 1
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((w, h, ow, oh, box, int((got != want).sum()) if got.shape == want.shape else "shape"))
    assert not bad, bad
    assert n == len(SHAPES) + 9 + 1                                       # 9 shapes have both sides over 20
