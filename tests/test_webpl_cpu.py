"""The lossless WebP decoder's host parse and arithmetic (ke_webpl_parse.h, ke_webpl_core.h) built for the CPU and held against
Pillow, bit for bit: taken files equal in pixels and mode, files of the test writer (tests/_vp8l_write.py: features forced)
equal, refusals with their status, caveats, and damaged files either refused or decoded as Pillow decodes them.  No GPU
needed: the headers are compiled with the host C++ compiler (tests/_webpl_cpu.cpp) into a temporary directory."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vp8l_write as V  # noqa: E402
import _webp_cases as W  # noqa: E402
import _webpl_cases as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _build(tmp_path_factory, name: str, flags: list):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp(name) / f"{name}.so")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-shared", "-fPIC", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "_webpl_cpu.cpp"), "-o", out])
    return out


def _load(path: str):
    lib = C.CDLL(path)
    lib.webpl_cpu_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.webpl_cpu_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return _load(_build(tmp_path_factory, "webpl_cpu", ["-O2"]))


@pytest.fixture(scope="module")
def written():
    return V.written_cases()


def probe(lib, data: bytes):
    """status, width, height, channels, EXIF / XMP present"""
    info = np.zeros(5, np.int32)
    lib.webpl_cpu_probe(data, len(data), info.ctypes.data)
    return tuple(int(v) for v in info)


def decode(lib, data: bytes):
    st, w, h, ch, _ = probe(lib, data)
    if st != L.OK:
        return st, None
    out = np.zeros((h, w, ch), np.uint8)
    st = lib.webpl_cpu_decode(data, len(data), out.ctypes.data)
    return st, out


def _assert_equal_pillow(lib, name, data):
    ref = L.pillow_pixels(data)
    assert ref is not None, name
    st, out = decode(lib, data)
    assert st == L.OK, name
    assert out.shape == ref.shape, (name, out.shape, ref.shape)     # the mode: RGB or RGBA as Pillow opens the file
    assert np.array_equal(out, ref), name


def test_taken_files_equal_pillow(cpu):
    assert len(L.golden_cases()) >= 24
    cases = L.taken_cases()
    modes = set()
    for name, data in cases:
        _assert_equal_pillow(cpu, name, data)
        modes.add(probe(cpu, data)[3])
    assert modes == {3, 4}


def test_encoder_settings_pillow_cannot_reach(cpu):
    lib = L.load_libwebp()
    if lib is None:
        pytest.skip("no libwebp encoder to load")
    for name, data in L.libwebp_cases(lib, seed=11, n=48):
        _assert_equal_pillow(cpu, name, data)


def test_writer_files_decode_in_pillow_to_what_went_in(written):
    """The writer's own check: Pillow is the judge of the files it makes."""
    for name, data, expected in written:
        ref = L.pillow_pixels(data)
        assert ref is not None, name
        assert np.array_equal(ref, expected[..., : ref.shape[2]]), name


def test_written_files_equal_pillow(cpu, written):
    assert len(written) >= 60
    for name, data, expected in written:
        _assert_equal_pillow(cpu, name, data)
        assert np.array_equal(decode(cpu, data)[1], expected[..., : probe(cpu, data)[3]]), name


def test_written_census(written):
    """Every feature the writer is there to force occurs at least once -- counted by the writer."""
    for k in sorted(V.CENSUS):
        print(f"{k:44s} {V.CENSUS[k]}")
    assert not [k for k in V.REQUIRED if V.CENSUS[k] == 0]
    assert V.CENSUS["entropy_image_groups_max"] >= 256


def test_refusals(cpu):
    for name, data, expected in L.refused_cases():
        st = decode(cpu, data)[0]
        assert st == expected, (name, st)
        assert probe(cpu, data)[0] in (expected, L.OK), name          # the header alone passes a stream that then ends early
    assert probe(cpu, L.refused_cases()[0][1])[0] == L.UNSUPPORTED


def test_caveats(cpu):
    """EXIF / XMP chunks are reported (an orientation may sit in either), and four channels where Pillow says RGBA."""
    for name, data in L.wrapped_cases():
        meta = any(t in (b"EXIF", b"XMP ") for t, _ in L.chunks(data))
        st, w, h, ch, m = probe(cpu, data)
        assert (st, m) == (L.OK, int(meta)), name
        assert ch == L.pillow_pixels(data).shape[2], name


def _fuzz(lib, count: int, seed: int):
    rng = np.random.default_rng(seed)
    bases = L.fuzz_bases()
    per = -(-count // len(bases))
    total = pillow_ok = taken = 0
    for base in bases:
        for data in L.damaged(base, rng, per):
            total += 1
            st, out = decode(lib, data)
            assert st in (L.OK, L.UNSUPPORTED, L.CORRUPT)
            ref = L.pillow_pixels(data)
            pillow_ok += ref is not None
            if st == L.OK:
                taken += 1
                assert ref is not None, f"mutation {total} decoded where Pillow refuses"
                assert out.shape == ref.shape and np.array_equal(out, ref), f"mutation {total} decoded where Pillow differs"
    return total, pillow_ok, taken


def test_damage_fuzz(cpu):
    """20 000 mutations: status 0 => Pillow decodes the file to the same pixels (so Pillow refusing => status != 0).  Not
    vacuous: Pillow itself decodes at least 1 000 of them (about 10 % expected), and the decoder takes at least half of those."""
    total, pillow_ok, taken = _fuzz(cpu, 20000, 2024)
    print(f"damage fuzz: {total} mutations, Pillow decodes {pillow_ok}, the decoder takes {taken}")
    assert total >= 20000 and pillow_ok >= 1000 and 2 * taken >= pillow_ok


def test_sanitised_build(tmp_path_factory):
    """The host code under AddressSanitizer and UBSan, as a program of its own (the sanitiser's runtime linked in): the
    refusals, the written files and 2 000 mutations -- statuses and pixels as Pillow's, and no report."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    work = tmp_path_factory.mktemp("webpl_san")
    exe = str(work / "webpl_san")
    base = [cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKE_WEBPL_MAIN", "-I", CSRC,
            os.path.join(ROOT, "tests", "_webpl_cpu.cpp"), "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    rng = np.random.default_rng(99)
    files = [(n, d, e) for n, d, e in L.refused_cases()] + [(n, d, L.OK) for n, d, _ in V.written_cases()]
    bases = L.fuzz_bases()
    files += [(f"mutation_{k}", d, None) for b in bases for k, d in enumerate(L.damaged(b, rng, -(-2000 // len(bases))))]
    paths = []
    for k, (_, data, _) in enumerate(files):
        paths.append(str(work / f"{k}.webp"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    lines = []
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    for at in range(0, len(paths), 500):
        done = subprocess.run([exe, *paths[at:at + 500]], env=env, capture_output=True, text=True)
        assert done.returncode == 0, done.stdout[-500:] + done.stderr[-4000:]
        lines += done.stdout.split("\n")[:-1]
    assert len(lines) == len(files)
    taken = 0
    for (name, data, expected), line, path in zip(files, lines, paths):
        st, w, h, ch = (int(v) for v in line.split())
        if expected is not None:
            assert st == expected, name
        if st == L.OK:
            ref = L.pillow_pixels(data)
            assert ref is not None and ref.shape == (h, w, ch), name
            assert np.array_equal(np.fromfile(path + ".out", np.uint8).reshape(h, w, ch), ref), name
            taken += expected is None
    print(f"sanitised build: {len(files)} files, {taken} mutations taken")
    assert len(files) >= 2000 + 60
