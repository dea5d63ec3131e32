"""The oversize refine route without a GPU: the reduced-size JPEG decode (ke_jpeg_core.h: the scaled geometry, jidctred's 4x4 /
2x2 / 1x1 transforms, upsampling at the reduced sizes) and Image.reduce (ke_reduce_core.h) compiled for the CPU
(tests/_jpeg_scaled_cpu.cpp) and held against the installed Pillow bit for bit; the whole chain -- draft scale, EXIF turn, reduce,
LANCZOS through the fractional box -- against the loader; formats.seam_actions with and without its ``oversize`` keyword; and a
sanitised program of its own over the whole decode and reduce sets."""
from __future__ import annotations

import ctypes as C
import io
import os
import shutil
import struct
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpeg_cases as J  # noqa: E402
import _jpeg_scaled_cases as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "_jpeg_scaled_cpu.cpp")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_scaled_cpu") / "jpeg_scaled_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-shared", "-fPIC", "-O2", "-I", CSRC, SOURCE, "-o", out])
    lib = C.CDLL(out)
    lib.jsc_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.jsc_probe.restype = None
    lib.jsc_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p]
    lib.jsc_reduce.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.jsc_reduce.restype = None
    return lib


def decode(lib, data: bytes, denom: int):
    """(status, pixels) of the file at 1 / denom"""
    info = np.zeros(4, np.int32)
    lib.jsc_probe(data, len(data), info.ctypes.data)
    st, w, h, ch = (int(v) for v in info)
    if st != 0:
        return st, None
    ow, oh = -(-w // denom), -(-h // denom)
    out = np.zeros((oh, ow) if ch == 1 else (oh, ow, ch), np.uint8)
    st = lib.jsc_decode(data, len(data), denom, out.ctypes.data)
    return st, out


def reduce(lib, a: np.ndarray, fx: int, fy: int) -> np.ndarray:
    h, w = a.shape[:2]
    a = np.ascontiguousarray(a)
    out = np.zeros((-(-h // fy), -(-w // fx), 3), np.uint8)
    lib.jsc_reduce(a.ctypes.data, w, h, fx, fy, out.ctypes.data)
    return out


def test_every_file_of_the_grid_equals_pillow_at_every_scale(cpu):
    files, reference = S.grid(), S.grid_reference()
    assert len(files) == len(S.SHAPES) * 2 * (len(S.SIDES) ** 2 + 1)
    ran_at = Counter()
    for (i, asked), (ref, ran) in reference.items():
        name, data = files[i]
        w, h = Image.open(io.BytesIO(data)).size
        if w >= asked and h >= asked:
            assert ran == asked, (name, asked, ran)            # the draft call forces the scale, read back from decoderconfig
        st, out = decode(cpu, data, ran)
        assert st == 0, (name, asked, st)
        assert out.shape == ref.shape, (name, asked, out.shape, ref.shape)
        assert np.array_equal(out, ref), (name, asked)
        ran_at[ran] += 1
    print("decodes per scale:", dict(ran_at))
    assert set(ran_at) == set(S.SCALES)


def test_scale_one_is_the_plain_decode(cpu):
    for name, data in S.grid()[::37]:
        st, out = decode(cpu, data, 1)
        assert st == 0 and np.array_equal(out, np.asarray(Image.open(io.BytesIO(data)))), name


def quantised_files():
    """(label, file bytes): files whose quantisation tables are overwritten with one value, small steps to the largest"""
    rng = np.random.default_rng(3)
    for value in (1, 2, 8, 16, 40, 64, 100, 160, 255):
        for sub in (0, 1, 2):
            for prog in (False, True):
                for kind in (0, 2):
                    yield (value, sub, prog, kind), J.with_quantisation_tables(
                        J._save(J._image(rng, 48, 40, kind), quality=95, subsampling=sub, progressive=prog), value)


def test_a_file_is_taken_with_pillows_pixels_or_handed_back_at_every_scale(cpu):
    """Quantisation tables overwritten with large steps push blocks out of the transforms' bound (ke_jpeg_core.h): whatever the
    scale, the file either decodes to Pillow's pixels or is handed back (status 1) -- and both happen."""
    seen = Counter()
    for label, data in quantised_files():
        for scale in S.SCALES:
            ref, ran = S.pillow_at_scale(data, scale)
            assert ran == scale
            st, out = decode(cpu, data, scale)
            assert st in (0, 1), (label, scale, st)
            if st == 0:
                assert np.array_equal(out, ref), (label, scale)
            seen[(scale, st)] += 1
    print("(scale, status):", dict(seen))
    assert all(seen[(s, st)] > 0 for s in S.SCALES for st in (0, 1))


def test_reduce_equals_pillow(cpu):
    """Every factor pair at every width and height in 1..20: each partial last column and row a factor can leave."""
    pairs, n = set(), 0
    for w, h, fx, fy, a in S.reduce_grid():
        ref = np.asarray(Image.fromarray(a).reduce((fx, fy)))
        out = reduce(cpu, a, fx, fy)
        assert out.shape == ref.shape and np.array_equal(out, ref), (w, h, fx, fy)
        pairs.add((fx, fy))
        n += 1
    assert {(fx, fy) for fx in range(1, 9) for fy in range(1, 9)} - {(1, 1)} <= pairs and (16, 16) in pairs
    assert n == len(S.REDUCE_PAIRS) * 400
    assert {c[:4] for c in S.reduce_cases()} <= {(w, h, fx, fy) for fx, fy in S.REDUCE_PAIRS for w in range(1, 21) for h in range(1, 21)}


TURNS = {3: Image.Transpose.ROTATE_180, 6: Image.Transpose.ROTATE_270, 8: Image.Transpose.ROTATE_90}


def chain(cpu, data: bytes, suffix: str, census: Counter):
    """The oversize route's steps on the CPU: the decode at the draft scale and the reduce are the headers under test; the turn
    and the resample through the box are Pillow's own calls here (the GPU tests hold the device's to them)."""
    m = S.CHAIN_MAX_SIDE
    if suffix == ".jpg":
        w, h = Image.open(io.BytesIO(data)).size
        scale = S.draft_scale(w, h, m)
        st, px = decode(cpu, data, scale)
        assert st == 0
        orientation = Image.open(io.BytesIO(data)).getexif().get(0x0112, 1)
    else:
        scale, orientation, px = 1, 1, np.asarray(Image.open(io.BytesIO(data)))
    census[("scale", scale)] += 1
    img = Image.fromarray(px)
    if orientation != 1:
        img = img.transpose(TURNS[orientation])
    w, h = img.size
    if max(w, h) <= m:
        return np.asarray(img)
    tw, th = S.thumbnail_size(w, h, m)
    fx, fy = S.reduce_factors(w, h, tw, th)
    census[("factors", fx, fy)] += 1
    if (fx, fy) == (1, 1):
        return np.asarray(img.resize((tw, th), Image.Resampling.LANCZOS, reducing_gap=None))
    small = Image.fromarray(reduce(cpu, np.asarray(img), fx, fy))
    return np.asarray(small.resize((tw, th), Image.Resampling.LANCZOS, box=(0, 0, w / fx, h / fy), reducing_gap=None))


def test_the_whole_chain_equals_the_loader(cpu, tmp_path):
    from kobato_eyes_amd.image_io import safe_load_image

    census = Counter()
    for name, suffix, data in S.chain_files():
        path = tmp_path / (name + suffix)
        path.write_bytes(data)
        ref = np.asarray(safe_load_image(path, max_side=S.CHAIN_MAX_SIDE))
        out = chain(cpu, data, suffix, census)
        assert out.shape == ref.shape, (name, suffix, out.shape, ref.shape)
        assert np.array_equal(out, ref), (name, suffix)
    print("census:", dict(census))
    assert {k[1] for k in census if k[0] == "scale"} == {1, 2, 4, 8}
    assert {k[1:] for k in census if k[0] == "factors"} >= S.CHAIN_FACTORS


def test_draft_scale_and_thumbnail_size_are_pillows():
    from kobato_eyes_amd import _native

    rng = np.random.default_rng(11)
    for _ in range(300):
        w, h, m = int(rng.integers(1, 3000)), int(rng.integers(1, 3000)), int(rng.integers(8, 300))
        im = Image.new("RGB", (w, h))
        b = io.BytesIO()
        if w * h < 40000:
            im.save(b, "JPEG")
            with Image.open(io.BytesIO(b.getvalue())) as f:
                f.draft("RGB", (m, m))
                f.load()
                assert int(_native.draft_scale([w], [h], m)[0]) == f.decoderconfig[0] == S.draft_scale(w, h, m)
        if max(w, h) > m:
            im.thumbnail((m, m))
            assert _native.thumbnail_size(w, h, m) == im.size == S.thumbnail_size(w, h, m)


def test_seam_actions_changes_only_the_oversize_cells():
    """Without the keyword: today's answers over the grid of test_refine_seams_cpu.py (and beyond its sides).  With it: only
    taken 3-channel files past the window change -- plain ones and those whose orientation the seam turns --, to SHRINK_OVERSIZE;
    RGBA, gray, refused files and images past the pixel bound stay with the loader."""
    import test_refine_seams_cpu as R
    from kobato_eyes_amd import formats as F

    m = R.MAX_SIDE
    changed = Counter()
    for kind in ("jpeg", "png", "tiff", "webp", "webpa"):
        rows = [k for _, k in R._files()]
        rows += [(0, st, c, g, o, w, h) for st in (0, 1) for c in (1, 3, 4) for g in range(4) for o in ((0, 1, 6, 9) if kind == "jpeg" else (0,))
                 for w, h in ((3 * m, 2 * m), (100, 4 * m + 1), (20000, 15000), (2 * m - 256, 2 * m - 256), (m, m), (2 * m - 257, 7))]
        _, st, c, g, o, w, h = (np.array(col, np.int32) for col in zip(*rows))
        flags = g | (o << 8)
        for seam in ("refine", "refine_parallel"):
            before = F.seam_actions(kind, seam, w, h, c, st, flags, m)
            off = F.seam_actions(kind, seam, w, h, c, st, flags, m, oversize=False)
            assert all(np.array_equal(a, b) for a, b in zip(before, off))
            on = F.seam_actions(kind, seam, w, h, c, st, flags, m, oversize=True)
            assert np.array_equal(on[1], before[1])                        # the orientations are as they were
            if seam == "refine_parallel":
                assert np.array_equal(on[0], before[0])
                continue
            orient = (flags >> 8) & 15
            plain = (c == 3) & ((flags & 3) == 0)
            turned = (c == 3) & ((flags & 3) == 1) & (orient >= 2) & (orient <= 8) & (kind == "jpeg")
            expect = (st == 0) & (np.maximum(w, h) >= 2 * m - 256) & (plain | turned) & (w.astype(np.int64) * h <= F.OVERSIZE_MAX_PIXELS)
            assert (before[0][expect] == F.LEAVE).all()
            assert np.array_equal(on[0], np.where(expect, F.SHRINK_OVERSIZE, before[0]))
            changed[kind] += int(expect.sum())
            assert not expect[(w.astype(np.int64) * h > F.OVERSIZE_MAX_PIXELS) | (c != 3) | (st != 0)].any()
    print("cells changed:", dict(changed))
    assert all(n > 0 for n in changed.values()) and changed["jpeg"] > changed["png"]      # the turned files are the JPEG row's
    assert 20000 * 15000 > F.OVERSIZE_MAX_PIXELS


def test_the_variable_is_off_unless_set_to_one(monkeypatch):
    from kobato_eyes_amd import formats as F

    monkeypatch.delenv("KE_GPU_REFINE_OVERSIZE", raising=False)
    assert not F.oversize_enabled()
    for value, on in (("0", False), ("", False), ("yes", False), ("1", True)):
        monkeypatch.setenv("KE_GPU_REFINE_OVERSIZE", value)
        assert F.oversize_enabled() is on


SANITISED_PARTS = 4


def test_sanitised_program(cpu, tmp_path):
    """The whole decode grid at every scale, the files of the IDCT-bound test (taken, or handed back by a reduced transform,
    as the plain build says) and the whole reduce grid through a program of its own built from the same headers with AddressSanitizer and UBSan: every
    buffer is exactly as large as its case says, so a read or write beyond is seen.  The cases are dealt to SANITISED_PARTS
    runs of the program, which run side by side."""
    exe = str(tmp_path / "jpeg_scaled_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-DJSC_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", CSRC, SOURCE, "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    files, reference = S.grid(), S.grid_reference()
    parts = [open(tmp_path / f"cases{k}.bin", "wb") for k in range(SANITISED_PARTS)]
    n = [0] * SANITISED_PARTS

    def case(head, data: bytes, want: bytes):
        k = sum(n) % SANITISED_PARTS
        parts[k].write(struct.pack("<7I", *head, len(data), len(want)) + data + want)
        n[k] += 1

    for (i, asked), (ref, ran) in reference.items():
        case((1, ran, 0, 0, 0), files[i][1], np.ascontiguousarray(ref).tobytes())
    assert sum(n) == len(files) * len(S.SCALES)
    handed_back = 0
    for (_, sub, _, _), data in quantised_files():
        for scale in S.SCALES:
            st, _ = decode(cpu, data, scale)
            if st == 1 and (scale == 1 or (scale == 2 and sub == 2)):
                continue                   # handed back by the 8x8 transform, which is the full-size decoder's and not part of this set
            case((1, scale, st, 0, 0), data, np.ascontiguousarray(S.pillow_at_scale(data, scale)[0]).tobytes() if st == 0 else b"")
            handed_back += st == 1
    assert handed_back > 0
    for w, h, fx, fy, a in S.reduce_grid():
        case((2, w, h, fx, fy), a.tobytes(), np.ascontiguousarray(np.asarray(Image.fromarray(a).reduce((fx, fy)))).tobytes())
    for f in parts:
        f.close()
    runs = [subprocess.Popen([exe, f.name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for f in parts]
    ends = [(r.communicate(), r.returncode) for r in runs]
    for k, ((out, err), code) in enumerate(ends):
        assert code == 0, (k, out[-2000:], err[-4000:])
        assert out.strip() == f"{n[k]} cases, 0 differ"
