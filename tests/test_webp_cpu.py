"""The lossy WebP decoder's host parse and arithmetic (ke_webp_parse.h, ke_webp_core.h) built for the CPU and held against
Pillow: taken files pixel-equal, refusals with their status, and damaged files either refused or decoded as Pillow decodes
them.  No GPU needed: the headers are compiled with the host C++ compiler (tests/_webp_cpu.cpp) into a temporary directory."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vp8_rewrite as R  # noqa: E402
import _webp_cases as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("webp_cpu") / "webp_cpu.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "_webp_cpu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.webp_cpu_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.webp_cpu_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def probe(lib, data: bytes):
    info = np.zeros(4, np.int32)
    lib.webp_cpu_probe(data, len(data), info.ctypes.data)
    return int(info[0]), int(info[1]), int(info[2]), int(info[3])


def decode(lib, data: bytes, yuv=False):
    st, w, h, _ = probe(lib, data)
    if st != W.OK:
        return st, None
    rgb = np.zeros((h, w, 3), np.uint8)
    planes = np.zeros(((w + 15) // 16) * ((h + 15) // 16) * 384, np.uint8) if yuv else None
    st = lib.webp_cpu_decode(data, len(data), rgb.ctypes.data, planes.ctypes.data if yuv else None)
    return st, (rgb, planes) if yuv else rgb


def test_taken_files_equal_pillow(cpu):
    cases = W.taken_cases()
    assert len(W.golden_cases()) >= 24
    for name, data in cases:
        st, rgb = decode(cpu, data)
        assert st == W.OK, name
        assert np.array_equal(rgb, W.pillow_rgb(data)), name


def test_encoder_settings_pillow_cannot_reach(cpu):
    lib = W.load_libwebp()
    if lib is None:
        pytest.skip("no libwebp encoder to load")
    for name, data in W.libwebp_cases(lib, seed=11, n=64):
        st, rgb = decode(cpu, data)
        assert st == W.OK, name
        assert np.array_equal(rgb, W.pillow_rgb(data)), name


def test_refusals(cpu):
    for name, data, expected in W.refused_cases():
        assert probe(cpu, data)[0] == expected, name
        assert decode(cpu, data)[0] == expected, name


def test_exif_and_xmp_are_reported(cpu):
    """Either chunk can hold an orientation Pillow's getexif() finds (XMP: tiff:Orientation) and exif_transpose applies."""
    for name, data in W.wrapped_cases() + [("xmp_orientation", W.xmp_turned_file())]:
        meta = any(t in (b"EXIF", b"XMP ") for t, _ in W.chunks(data))
        assert probe(cpu, data)[3] == int(meta), name
    from PIL import Image, ImageOps
    import io

    with Image.open(io.BytesIO(W.xmp_turned_file())) as im:
        assert ImageOps.exif_transpose(im).size == im.size[::-1]            # the reason it is reported


def _libwebp_yuv():
    lib = W.load_libwebp()
    if lib is None:
        pytest.skip("no libwebp to load")
    lib.WebPDecodeYUV.restype = C.c_void_p
    lib.WebPDecodeYUV.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _assert_yuv_planes_equal(cpu, lib, name, data):
    st, (rgb, planes) = decode(cpu, data, yuv=True)
    assert st == W.OK, name
    w, h, u, v, stride, uv_stride = (C.c_int() for _ in range(6))
    uu, vv = C.c_void_p(), C.c_void_p()
    y = lib.WebPDecodeYUV(data, len(data), C.byref(w), C.byref(h), C.byref(uu), C.byref(vv), C.byref(stride), C.byref(uv_stride))
    assert y, name
    try:
        W_, H_ = w.value, h.value
        mb_w, mb_h = (W_ + 15) // 16, (H_ + 15) // 16
        ys = 16 * mb_w
        Y = planes[: mb_w * mb_h * 256].reshape(16 * mb_h, ys)[:H_, :W_]
        U = planes[mb_w * mb_h * 256: mb_w * mb_h * 320].reshape(8 * mb_h, 8 * mb_w)[: (H_ + 1) // 2, : (W_ + 1) // 2]
        V = planes[mb_w * mb_h * 320:].reshape(8 * mb_h, 8 * mb_w)[: (H_ + 1) // 2, : (W_ + 1) // 2]
        ref_y = np.array([np.frombuffer(C.string_at(y + r * stride.value, W_), np.uint8) for r in range(H_)])
        ref_u = np.array([np.frombuffer(C.string_at(uu.value + r * uv_stride.value, (W_ + 1) // 2), np.uint8) for r in range((H_ + 1) // 2)])
        ref_v = np.array([np.frombuffer(C.string_at(vv.value + r * uv_stride.value, (W_ + 1) // 2), np.uint8) for r in range((H_ + 1) // 2)])
        assert np.array_equal(Y, ref_y) and np.array_equal(U, ref_u) and np.array_equal(V, ref_v), name
    finally:
        lib.WebPFree(C.c_void_p(y))


def test_yuv_planes_equal_libwebp(cpu):
    lib = _libwebp_yuv()
    for name, data in W.pillow_cases(seed=5, n=40) + W.golden_cases():
        _assert_yuv_planes_equal(cpu, lib, name, data)


def test_damage_fuzz(cpu):
    """20 000 mutations: whatever the decoder takes, Pillow decodes to the same pixels."""
    rng = np.random.default_rng(2024)
    bases = [d for _, d in W.pillow_cases(seed=7, n=20) if len(d) > 40] + [d for _, d in W.golden_cases()[:10]]
    per = -(-20000 // len(bases))
    taken = total = 0
    for base in bases:
        for data in W.damaged(base, rng, per):
            total += 1
            st, rgb = decode(cpu, data)
            assert st in (W.OK, W.UNSUPPORTED, W.CORRUPT)
            if st == W.OK:
                taken += 1
                ref = W.pillow_rgb(data)
                assert ref is not None and np.array_equal(rgb, ref), f"mutation {total} decoded where Pillow differs"
    assert total >= 20000 and taken > 1000


# ---- rewritten key frames (tests/_vp8_rewrite.py): header fields and modes no encoder writes, Pillow still the reference ----
@pytest.fixture(scope="module")
def rewritten():
    return {g: fn() for g, fn in R.GROUPS.items()}


def test_rewriter_identity():
    """emit(parse(f)) decodes in Pillow to exactly the pixels of f, and parses back to the same values."""
    for name, data in W.taken_cases():
        f = R.parse(data)
        out = R.emit(f, f.container)
        assert np.array_equal(W.pillow_rgb(out), W.pillow_rgb(data)), name
        assert R.encoded_fields(R.parse(out)) == R.encoded_fields(f), name


def test_rewritten_files_parse_back(rewritten):
    for group, cases in rewritten.items():
        for name, data, f in cases:
            assert R.encoded_fields(R.parse(data)) == R.encoded_fields(f), name


def _decode_against_pillow(cpu, name, data):
    """(status, equal to Pillow); a file Pillow refuses must not come back OK, and probe agrees with the decode (the header
    alone passes a file the tokens then refuse for the coefficient limit)."""
    ref = W.pillow_rgb(data)
    st, rgb = decode(cpu, data)
    pst, w, h, meta = probe(cpu, data)
    assert pst == st or (pst, st) == (W.OK, W.UNSUPPORTED), name
    if ref is None:
        assert st != W.OK, f"{name}: decoded where Pillow refuses"
        return st, False
    if st == W.OK:
        assert (h, w, meta) == (*ref.shape[:2], 0), name
    return st, st == W.OK and np.array_equal(rgb, ref)


def test_rewritten_bases_are_taken(cpu):
    """What the groups start from decodes, and equals Pillow, before any rewriting."""
    bases = R._bases(21) + R._bases(22, golden_every=3) + R._bases(23, golden_every=3) + R._bases(24)
    bases += R.pillow_bases(124, quality=(90, 101), sizes=R.BASE_SIZES[:12])
    bases += R.pillow_bases(25, kinds=("noisy", "drawing"), quality=(85, 96), sizes=R.BASE_SIZES[3:16])
    for name, data in bases:
        assert _decode_against_pillow(cpu, name, data) == (W.OK, True), name


@pytest.mark.parametrize("group", ["modes", "filter", "header", "quant_down"])
def test_rewritten_files_equal_pillow(cpu, rewritten, group):
    """No exemptions: the coefficients, and so the decoder's limit, are those of a base that was taken."""
    cases = rewritten[group]
    assert len(cases) >= 60
    for name, data, _ in cases:
        assert _decode_against_pillow(cpu, name, data) == (W.OK, True), name


def test_quant_up_files_equal_pillow_or_go_to_pillow(cpu, rewritten):
    """Quantisers raised up to 127: a file either decodes to Pillow's pixels or is refused (the dequantised limit) and
    left to Pillow, which decodes it."""
    taken = refused = 0
    for name, data, _ in rewritten["quant_up"]:
        st, equal = _decode_against_pillow(cpu, name, data)
        assert st in (W.OK, W.UNSUPPORTED), name
        if st == W.OK:
            assert equal, name
            taken += 1
        else:
            assert W.pillow_rgb(data) is not None, name
            refused += 1
    print(f"quant_up: {taken} taken, {refused} refused")
    assert taken >= 10 and refused >= 10


def test_rewritten_yuv_planes_equal_libwebp(cpu, rewritten):
    lib = _libwebp_yuv()
    for group, cases in rewritten.items():
        for name, data, _ in cases[::4]:
            if decode(cpu, data)[0] == W.OK:
                _assert_yuv_planes_equal(cpu, lib, name, data)


def test_rewritten_census(rewritten):
    """Every header field value the encoders never write, every effective filter level and sharpness, and every
    (predictor, position class) pair occurs in the rewritten corpus."""
    c = R.census([case for cases in rewritten.values() for case in cases])
    for k, v in c.items():
        print(f"{k:40s} {v}")
    assert not [k for k, v in c.items() if v == 0]
