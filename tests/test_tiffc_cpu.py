"""The host parse and the stream arithmetic of the decoder for LZW and PackBits TIFF files (ke_tiffc_parse.h, ke_tiffc_core.h, and
the uncompressed parser they build on) compiled for the CPU and held against Pillow / libtiff, bit for bit: every valid file
taken with Pillow's shape and bytes, the refusals with their status, and damaged files either refused or decoded as Pillow
decodes them.  No GPU needed: the headers are compiled with the host C++ compiler (tests/_tiffc_cpu.cpp) into a temporary
directory."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lzw_write as Z  # noqa: E402
import _tiff_cases as T  # noqa: E402
import _tiffc_cases as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tiffc_cpu") / "tiffc_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-shared", "-fPIC", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "_tiffc_cpu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.tiffc_cpu_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.tiffc_cpu_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.tiffc_cpu_probe_plain.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.tiffc_cpu_strip_records.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return lib


def probe(lib, data: bytes):
    """status, width, height, channels, compression, predictor, strips, rows per strip"""
    info = np.zeros(8, np.int32)
    lib.tiffc_cpu_probe(data, len(data), info.ctypes.data)
    return tuple(int(v) for v in info)


def decode(lib, data: bytes):
    st, w, h, ch = probe(lib, data)[:4]
    if st != A.OK:
        return st, None
    out = np.zeros((h, w) if ch == 1 else (h, w, ch), np.uint8)
    st = lib.tiffc_cpu_decode(data, len(data), out.ctypes.data)
    return st, out


def _assert_equal_pillow(lib, name, data):
    ref = A.pillow_pixels(data)
    assert ref is not None, name
    st, out = decode(lib, data)
    assert st == A.OK, (name, st)
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert np.array_equal(out, ref), name


def test_the_writers_round_trip():
    """The tests' own LZW writer against a plain reader of the same rules, and its PackBits writer: what goes in comes out."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 300, 9000):
        data = A._run_heavy(rng, n)
        for how in ({}, dict(clear_at=4096), dict(clear_every=50), dict(eoi=False)):
            codes = Z.codes_of(data, **how)
            table, out, prev = {}, bytearray(), None
            for c in codes:
                if c == Z.CLEAR:
                    table, prev = {}, None
                    continue
                if c == Z.EOI:
                    break
                s = bytes([c]) if c < 256 else table[c] if c in table else prev + prev[:1]
                if prev is not None and Z.FIRST + len(table) < 4096:
                    table[Z.FIRST + len(table)] = prev + s[:1]
                out += s
                prev = s
            assert bytes(out) == data, (n, how)
        packed, k, back = Z.packbits(data), 0, bytearray()
        while k < len(packed):
            h = packed[k]
            if h < 128:
                back += packed[k + 1:k + 2 + h]
                k += 2 + h
            else:
                back += packed[k + 1:k + 2] * (257 - h)
                k += 2
        assert bytes(back) == data


def test_pillow_written_files_equal_pillow(cpu):
    cases = A.pillow_cases()
    seen = Counter()
    for name, data in cases:
        _assert_equal_pillow(cpu, name, data)
        st, w, h, ch, comp, pred, nstrips, _ = probe(cpu, data)
        seen[(comp, pred, ch)] += 1
        seen["many_strips"] += nstrips > 1
    print("Pillow's files by (compression, predictor, channels):", dict(seen))
    # (libtiff's PackBits codec does not know the Predictor tag: those files are written and read back undifferenced)
    assert all(seen[(A.LZW, p, ch)] > 0 and seen[(A.PACKBITS, 1, ch)] > 0 for p in (1, 2) for ch in (1, 3, 4)) and seen["many_strips"] > 0
    assert len(cases) == 4 * 2 * 2 * len(A.SIZES)


def test_handmade_directories_equal_pillow(cpu):
    for name, data in A.handmade_cases():
        _assert_equal_pillow(cpu, name, data)


def test_streams_libtiff_never_writes_equal_pillow(cpu):
    cases = A.lzw_stream_cases() + A.packbits_stream_cases()
    for name, data in cases:
        _assert_equal_pillow(cpu, name, data)
    assert len(cases) > 40


def test_the_copy_patterns_of_the_gif_streams_equal_pillow(cpu):
    """Runs of every distance 2..17 and last strings cut to one byte (tests/_gif_stream_cases.tiff_strips) as LZW strips: the
    direct decode equals Pillow, and so does the kernels' way on the host -- the strip through the sink the two LZW walkers
    share (csrc/ke_lz_records.h), its records made in order byte by byte.  That the strips hold what they are named for is
    counted from those records: a run of the longest kind at every distance 2..16, contiguous copies at 17, phase 0 at 3, 7,
    15 and 16, runs continued at lane 0, records into the slack."""
    import _gif_stream_cases as S

    cases = A.sink_cases()
    census = Counter()
    for name, data in cases:
        _assert_equal_pillow(cpu, name, data)
        ref = A.pillow_pixels(data)
        plane = np.zeros(ref.size + 2, np.uint8)
        rec = np.zeros((ref.size // 2 + 2, 2), np.uint32)
        n, want = C.c_uint32(), C.c_uint32()
        assert cpu.tiffc_cpu_strip_records(data, len(data), 0, plane.ctypes.data, rec.ctypes.data, C.byref(n), C.byref(want)) == A.OK, name
        assert want.value == ref.size and n.value <= ref.size // 2 + 2, name
        for dst, word in rec[:n.value].tolist():
            for k in range((word & 511) + 2):
                plane[dst + k] = plane[dst + k - (word >> 9)]
        assert np.array_equal(plane[:ref.size], ref.ravel()), name
        census += S.records_census(rec[:n.value], ref.size)
    missing = [f for f in [f"run_d{d}_of_{S.longest_run(d)}_copies" for d in range(2, 17)] + [f"run_d{d}_phase_0" for d in (3, 7, 15, 16)] +
               [f"run_d{d}_continued_at_lane_0" for d in range(3, 17)] + ["contiguous_copies_at_distance_17", "record_into_the_slack", "run_behind_a_blocker"]
               if not census[f]]
    assert not missing, missing
    assert len(cases) >= 140


def test_every_valid_file_is_taken(cpu):
    """All families in one sweep: 0 refused."""
    count = Counter()
    refused = []
    for family, name, data in A.valid_cases():
        count[family] += 1
        if decode(cpu, data)[0] != A.OK:
            refused.append((name, probe(cpu, data)[0]))
    print("valid files per family:", dict(count))
    assert not refused, refused[:5]
    assert all(count[f] > 0 for f in ("pillow", "handmade", "lzw_streams", "packbits_streams"))


def test_refusals(cpu):
    """The status per file; what is expected as CORRUPT is what Pillow raises on."""
    for name, data, expected in A.refused_cases():
        st = decode(cpu, data)[0]
        assert st == expected, (name, st)
        if expected == A.CORRUPT:
            assert A.pillow_pixels(data) is None, name


def test_late_change_streams_are_refused_or_equal_to_pillow(cpu):
    for name, data in A.late_change_cases():
        st, out = decode(cpu, data)
        ref = A.pillow_pixels(data)
        if st == A.OK:
            assert ref is not None and out.shape == ref.shape and np.array_equal(out, ref), name
        if st == A.CORRUPT:
            assert ref is None, name


def test_the_uncompressed_parser_answers_as_before(cpu):
    """ke_parse_tiff over the uncompressed cases of tests/_tiff_cases.py and over the compressed files: the former as their
    expectations say, the latter all refused (status 1), as before the directory reading was shared."""
    info = np.zeros(4, np.int32)
    for name, data, ref in list(T.supported()) + list(T.handmade()):
        cpu.tiffc_cpu_probe_plain(data, len(data), info.ctypes.data)
        left = ref is None or any(name.startswith(p) for p in T.LEFT_TO_PILLOW)
        assert (info[0] != 0) == left, name
        if not left:
            assert (info[2], info[1]) == ref.shape[:2], name
        assert decode(cpu, data)[0] != A.OK, name                   # and none of them is the new decoder's
    for name, data, expected in T.refused():
        cpu.tiffc_cpu_probe_plain(data, len(data), info.ctypes.data)
        assert info[0] == expected, name
    for _, name, data in A.valid_cases():
        cpu.tiffc_cpu_probe_plain(data, len(data), info.ctypes.data)
        assert info[0] == 1, name


def _fuzz(lib):
    census = {c: Counter() for c in (A.LZW, A.PACKBITS)}
    for k, (comp, data) in enumerate(A.damaged_set()):
        st, out = decode(lib, data)
        assert st in (A.OK, A.UNSUPPORTED, A.CORRUPT)
        ref = A.pillow_pixels(data)
        census[comp]["cases"] += 1
        census[comp]["pillow"] += ref is not None
        if st == A.OK:
            census[comp]["taken"] += 1
            assert ref is not None, f"damaged file {k} (compression {comp}) decoded where Pillow raises"
            assert out.shape == ref.shape and np.array_equal(out, ref), f"damaged file {k} (compression {comp}) decoded where Pillow differs"
    return census


def test_damage_fuzz(cpu):
    """5 600 damaged files (14 bases x 400: directory bytes, strip bits / bytes / stretches, cuts, byte counts): status 0 => strict
    Pillow decodes the file to the same pixels (so Pillow raising => status != 0).  Both outcomes occur: of the LZW files
    Pillow takes 995 of 2 800 and the decoder 940, of the PackBits files 1 652 of 2 800 and 1 605 (the first run; printed every
    run).  What the decoder leaves of Pillow's is damage to the directory that the tighter whitelist refuses.  The floors
    asserted are 20 % under that census -- 750 and 1 280 -- so refusing everything does not pass."""
    census = _fuzz(cpu)
    for comp, c in census.items():
        print(f"damage census, compression {comp}: {c['cases']} cases, Pillow takes {c['pillow']}, the decoder takes {c['taken']}")
    assert sum(c["cases"] for c in census.values()) >= 5000
    assert census[A.LZW]["taken"] >= 750 and census[A.PACKBITS]["taken"] >= 1280
    assert all(0 < c["pillow"] < c["cases"] for c in census.values())


def test_sanitised_build(tmp_path_factory):
    """The host code under AddressSanitizer and UBSan, as a program of its own: the refusals, the hand-made streams and 1 400
    mutations -- statuses and pixels as Pillow's, and no report."""
    cxx = _cxx()
    work = tmp_path_factory.mktemp("tiffc_san")
    exe = str(work / "tiffc_san")
    base = [cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKE_TIFFC_MAIN", "-I", CSRC,
            os.path.join(ROOT, "tests", "_tiffc_cpu.cpp"), "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    rng = np.random.default_rng(99)
    files = [(n, d, e) for n, d, e in A.refused_cases()] + [(n, d, A.OK) for n, d in A.lzw_stream_cases() + A.packbits_stream_cases() + A.handmade_cases()]
    files += [(n, d, None) for n, d in A.late_change_cases()]
    files += [(f"mutation_{k}", d, None) for _, b in A.fuzz_bases() for k, d in enumerate(A.damaged(b, rng, 100))]
    paths = []
    for k, (_, data, _) in enumerate(files):
        paths.append(str(work / f"{k}.tif"))
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
            shape = (h, w) if ch == 1 else (h, w, ch)
            assert ref is not None and ref.shape == shape, name
            assert np.array_equal(np.fromfile(path + ".out", np.uint8).reshape(shape), ref), name
            taken += expected is None
    print(f"sanitised build: {len(files)} files, {taken} mutations taken")
    assert len(files) >= 1400 + 100
