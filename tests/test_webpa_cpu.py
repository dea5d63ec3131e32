"""The host parse and arithmetic of the decoder for lossy WebP files with an alpha plane (ke_webpa_parse.h, ke_webpa_core.h, and
the lossy and lossless decoders' headers they join) built for the CPU and held against Pillow, bit for bit: every taken file
equal in mode, size and every byte, the refusals with their status, caveats, and damaged files either refused or decoded as
Pillow decodes them.  No GPU needed: the headers are compiled with the host C++ compiler (tests/_webpa_cpu.cpp) into a
temporary directory."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import shutil
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _webpa_cases as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("webpa_cpu") / "webpa_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-shared", "-fPIC", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "_webpa_cpu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.webpa_cpu_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.webpa_cpu_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.webpa_cpu_unfilter.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return lib


def probe(lib, data: bytes):
    """status, width, height, channels, EXIF / XMP present, method, filter, pre-processing"""
    info = np.zeros(8, np.int32)
    lib.webpa_cpu_probe(data, len(data), info.ctypes.data)
    return tuple(int(v) for v in info)


def decode(lib, data: bytes):
    st, w, h = probe(lib, data)[:3]
    if st != A.OK:
        return st, None
    out = np.zeros((h, w, 4), np.uint8)
    st = lib.webpa_cpu_decode(data, len(data), out.ctypes.data)
    return st, out


def _assert_equal_pillow(lib, name, data):
    ref = A.pillow_pixels(data)
    assert ref is not None, name
    st, out = decode(lib, data)
    assert st == A.OK, (name, st)
    assert out.shape == ref.shape, (name, out.shape, ref.shape)     # the mode: Pillow opens the file as RGBA
    assert np.array_equal(out, ref), name


def test_inverse_filters_equal_the_tests_restatement(cpu):
    rng = np.random.default_rng(1)
    for w, h in ((1, 1), (1, 8), (8, 1), (13, 7), (64, 33)):
        for filt in range(4):
            a = A.plane(rng, w, h, A.ALPHA_KINDS[(w + filt) % 5])
            stored = A.forward_filter(a, filt)
            assert np.array_equal(A.inverse_filter(stored, filt), a), (w, h, filt)          # the test's own two halves agree
            out = np.zeros_like(a)
            cpu.webpa_cpu_unfilter(filt, np.ascontiguousarray(stored).ctypes.data, out.ctypes.data, w, h)
            assert np.array_equal(out, a), (w, h, filt)


def test_pillow_written_files_equal_pillow(cpu):
    """Family 1: every header byte Pillow writes here occurs, and sizes reach from 1 x 1 past 512 x 512."""
    cases = A.pillow_cases()
    bytes_seen = Counter()
    for name, data in cases:
        _assert_equal_pillow(cpu, name, data)
        bytes_seen[A.header_byte(data)] += 1
    print("ALPH header bytes of Pillow's files:", {hex(k): v for k, v in sorted(bytes_seen.items())})
    assert {0x00, 0x01, 0x05, 0x11} <= set(bytes_seen)
    sizes = [A.pillow_pixels(d).shape[:2] for _, d in cases]
    assert (1, 1) in sizes and max(h * w for h, w in sizes) >= 512 * 512


def test_encoder_settings_pillow_cannot_reach(cpu):
    """Family 2: the libwebp encoder's alpha_compression / alpha_filtering / alpha_quality."""
    lib = A.load_libwebp()
    if lib is None:
        pytest.skip("no libwebp encoder to load (family 3 holds the same ground: every method and filter)")
    seen = Counter()
    for name, data in A.libwebp_cases(lib):
        _assert_equal_pillow(cpu, name, data)
        seen[A.header_byte(data)] += 1
    print("ALPH header bytes of the encoder's files:", {hex(k): v for k, v in sorted(seen.items())})
    assert {b & 3 for b in seen} == {0, 1}


def test_hand_muxed_files_equal_pillow_and_the_intended_plane(cpu):
    """Family 3: Pillow's alpha is the plane that went in (so the test's muxer and filters are right), and the decoder's
    pixels are Pillow's."""
    cases = A.muxed_cases()
    combos = Counter()
    for name, data, want in cases:
        ref = A.pillow_pixels(data)
        assert ref is not None and ref.shape[2] == 4, name
        assert np.array_equal(ref[..., 3], want), name
        _assert_equal_pillow(cpu, name, data)
        st, _, _, _, _, method, filt, pre = probe(cpu, data)
        combos[(method, filt)] += 1
        combos[("pre", pre)] += 1
    print("method x filter of the hand-muxed files:", dict(combos))
    assert all(combos[(m, f)] > 0 for m in (0, 1) for f in range(4)) and combos[(-1, 0)] > 0 and combos[("pre", 1)] > 0


def test_committed_files_equal_pillow_and_their_recorded_pixels(cpu):
    """Family 5: the sha256 recorded with the file is of Pillow's pixels then, and the decoder's now."""
    cases = A.golden_cases()
    assert len(cases) >= 36
    for name, data, sha in cases:
        _assert_equal_pillow(cpu, name, data)
        assert hashlib.sha256(decode(cpu, data)[1].tobytes()).hexdigest() == sha, name


def test_census():
    """Every family is present (2 only where the encoder can be loaded)."""
    lib = A.load_libwebp()
    count = Counter(f for f, _, _ in A.all_taken(lib))
    count[4] = len(A.refused_cases())
    print("files per family:", dict(sorted(count.items())))
    assert all(count[f] > 0 for f in (1, 3, 4, 5)) and (lib is None or count[2] > 0)


def test_every_taken_file_is_taken(cpu):
    """Families 1-3 and 5 in one sweep: 0 refused."""
    refused = [(n, probe(cpu, d)[0]) for _, n, d in A.all_taken(A.load_libwebp()) if decode(cpu, d)[0] != A.OK]
    assert not refused, refused[:5]


def test_refusals(cpu):
    """Family 4: the status per file; what is expected as CORRUPT is what Pillow fails on."""
    for name, data, expected in A.refused_cases():
        st = decode(cpu, data)[0]
        assert st == expected, (name, st)
        if expected == A.CORRUPT:
            assert A.pillow_pixels(data) is None, name
    pixels = A.pillow_pixels(dict((n, d) for n, d, _ in A.refused_cases())["alph_without_flag"])
    assert pixels is not None                                       # Pillow opens it; its alpha is not the chunk's plane


def test_caveats(cpu):
    """EXIF / XMP chunks are reported (an orientation may sit in either); four channels throughout."""
    seen = set()
    for name, data, _ in A.container_cases():
        meta = any(t in (b"EXIF", b"XMP ") for t, _ in A.chunks(data))
        st, w, h, ch, m = probe(cpu, data)[:5]
        assert (st, ch, m) == (A.OK, 4, int(meta)), name
        seen.add(m)
    assert seen == {0, 1}


def _fuzz(lib, count: int, seed: int):
    rng = np.random.default_rng(seed)
    bases = A.fuzz_bases()
    per = -(-count // len(bases))
    total = pillow_ok = taken = 0
    for base in bases:
        for data in A.damaged(base, rng, per):
            total += 1
            st, out = decode(lib, data)
            assert st in (A.OK, A.UNSUPPORTED, A.CORRUPT)
            ref = A.pillow_pixels(data)
            pillow_ok += ref is not None
            if st == A.OK:
                taken += 1
                assert ref is not None, f"mutation {total} decoded where Pillow refuses"
                assert out.shape == ref.shape and np.array_equal(out, ref), f"mutation {total} decoded where Pillow differs"
    return total, pillow_ok, taken


def test_damage_fuzz(cpu):
    """20 000 mutations between offset 12 and the end of the ALPH chunk: status 0 => Pillow decodes the file to the same
    pixels (so Pillow refusing => status != 0).  Not vacuous: Pillow itself decodes at least a quarter of them (the first run:
    5 987 of 20 016, 30 %).  The take rate among those is printed; the first run gave 5 533 of 5 987 (92 %) -- what is left out
    is mostly damage after which Pillow still opens the file as something this decoder does not reproduce: a cleared VP8X
    alpha flag or a broken ALPH tag (the demuxer drops or skips the chunk), a changed flag byte or canvas -- and the floor
    asserted here is three quarters of what Pillow decodes, a margin of 17 points under that run."""
    total, pillow_ok, taken = _fuzz(cpu, 20000, 2025)
    print(f"damage fuzz: {total} mutations, Pillow decodes {pillow_ok}, the decoder takes {taken}")
    assert total >= 20000 and 4 * pillow_ok >= total and 4 * taken >= 3 * pillow_ok


def test_sanitised_build(tmp_path_factory):
    """The host code under AddressSanitizer and UBSan, as a program of its own: the refusals, the hand-muxed files and 2 400
    mutations -- statuses and pixels as Pillow's, and no report."""
    cxx = _cxx()
    work = tmp_path_factory.mktemp("webpa_san")
    exe = str(work / "webpa_san")
    base = [cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKE_WEBPA_MAIN", "-I", CSRC,
            os.path.join(ROOT, "tests", "_webpa_cpu.cpp"), "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    rng = np.random.default_rng(98)
    files = [(n, d, e) for n, d, e in A.refused_cases()] + [(n, d, A.OK) for n, d, _ in A.muxed_cases()]
    bases = A.fuzz_bases()
    files += [(f"mutation_{k}", d, None) for b in bases for k, d in enumerate(A.damaged(b, rng, 100))]
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
        if st == A.OK:
            ref = A.pillow_pixels(data)
            assert ref is not None and ref.shape == (h, w, ch), name
            assert np.array_equal(np.fromfile(path + ".out", np.uint8).reshape(h, w, ch), ref), name
            taken += expected is None
    print(f"sanitised build: {len(files)} files, {taken} mutations taken")
    assert len(files) >= 2400 + 100
