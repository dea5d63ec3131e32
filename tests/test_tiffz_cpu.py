"""The host parse of the decoder for deflate-compressed TIFF files and the arithmetic its kernels run (ke_tiffz_parse.h,
ke_tiffz_core.h, ke_png_core.h's inflate, and the two TIFF parsers they build on) compiled for the CPU and held against Pillow /
libtiff, bit for bit: every valid file taken with Pillow's shape and bytes, the refusals with their status, the two places
where the decoder is stricter than libtiff by name, damaged files either refused or decoded as Pillow decodes them; the three
TIFF probes against each other; the records route and the Adler sum by lanes; the format table's row.  No GPU needed: the
headers are compiled with the host C++ compiler (tests/_tiffz_cpu.cpp) into a temporary directory."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import sys
import zlib
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiff_cases as T  # noqa: E402
import _tiffc_cases as A  # noqa: E402
import _tiffz_cases as Z  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tiffz_cpu") / "tiffz_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-shared", "-fPIC", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "_tiffz_cpu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.tiffz_cpu_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.tiffz_cpu_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.tiffz_cpu_probe_other.argtypes = [C.c_char_p, C.c_uint64, C.c_int32]
    lib.tiffz_cpu_strip_records.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p] + [C.POINTER(C.c_uint32)] * 3
    lib.tiffz_cpu_adler_by_lanes.argtypes = [C.c_void_p, C.c_uint32]
    lib.tiffz_cpu_adler_by_lanes.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def valid():
    return Z.valid_cases()


def probe(lib, data: bytes):
    """status, width, height, channels, compression, predictor, strips, rows per strip"""
    info = np.zeros(8, np.int32)
    lib.tiffz_cpu_probe(data, len(data), info.ctypes.data)
    return tuple(int(v) for v in info)


def decode(lib, data: bytes):
    st, w, h, ch = probe(lib, data)[:4]
    if st != Z.OK:
        return st, None
    out = np.zeros((h, w) if ch == 1 else (h, w, ch), np.uint8)
    st = lib.tiffz_cpu_decode(data, len(data), out.ctypes.data)
    return st, out


def _assert_equal_pillow(lib, name, data):
    ref = Z.pillow_pixels(data)
    assert ref is not None, name
    st, out = decode(lib, data)
    assert st == Z.OK, (name, st)
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert np.array_equal(out, ref), name


def test_pillow_written_files_equal_pillow(cpu):
    cases = Z.pillow_cases()
    seen = Counter()
    for name, data in cases:
        _assert_equal_pillow(cpu, name, data)
        st, w, h, ch, comp, pred, nstrips, _ = probe(cpu, data)
        seen[(comp, pred, ch)] += 1
        seen["many_strips"] += nstrips > 1
    print("Pillow's files by (compression, predictor, channels):", dict(seen))
    # (libtiff writes Compression 8 under both names; files that say 32946 are among the hand-made ones)
    assert all(seen[(Z.DEFLATE, p, ch)] > 0 for p in (1, 2) for ch in (1, 3, 4)) and seen["many_strips"] > 0
    assert len(cases) == 4 * 2 * 2 * len(A.SIZES)


def test_handmade_directories_equal_pillow(cpu):
    cases = Z.handmade_cases()
    for name, data in cases:
        _assert_equal_pillow(cpu, name, data)
    assert len(cases) == 3 * 2 * 2 * 15


def test_streams_no_compressor_writes_equal_pillow(cpu):
    named = Z.named_stream_cases()
    for name, data in named + Z.png_stream_cases():
        _assert_equal_pillow(cpu, name, data)
    names = {n for n, _ in named}
    assert {"code_of_15_bits", "single_code_distance_tree", "every_block_type_behind_every_bit_offset", "empty_stored_block",
            "match_of_258_at_distance_1", "match_at_distance_32768", "chain_of_100_dependent_copies"} <= names
    assert all(f"want_mod_4_is_{k}_ends_in_{how}" in names for k in range(4) for how in ("literal", "copy"))
    st, w, h, ch, comp, pred, nstrips, rows = probe(cpu, dict(named)["match_at_distance_32768"])
    assert (w, h, nstrips) == (331, 100, 1) and w * h >= 32771


def test_what_libtiff_does_with_odd_strips(cpu):
    """Every row of the table with its status.  Status 0: Pillow's pixels.  Status 2: Pillow raises -- except the rows named in
    STRICTER_THAN_LIBTIFF, which Pillow opens with the intended pixels (libtiff stops inflating when the strip is full; the
    decoder wants one complete stream that yields exactly the strip) and which therefore go to Pillow at every seam."""
    stricter = set()
    for name, data, expected, opens in Z.odd_strip_cases():
        st, out = decode(cpu, data)
        assert st == expected, (name, st)
        ref = Z.pillow_pixels(data)
        assert (ref is not None) == opens, name
        if st == Z.OK:
            assert np.array_equal(out, ref), name
        elif opens:
            stricter.add(next(s for s in Z.STRICTER_THAN_LIBTIFF if name.startswith(s)))
    assert stricter == set(Z.STRICTER_THAN_LIBTIFF)


def test_every_valid_file_is_taken(cpu, valid):
    count = Counter()
    refused = []
    for family, name, data in valid:
        count[family] += 1
        if decode(cpu, data)[0] != Z.OK:
            refused.append((name, probe(cpu, data)[0]))
    print("valid files per family:", dict(count))
    assert not refused, refused[:5]
    assert all(count[f] > 0 for f in ("pillow", "handmade", "named_streams", "png_streams", "odd_strips"))


def test_refusals(cpu):
    """The status per file; what is expected as CORRUPT is what Pillow raises on.  Orientation and unknown tags stay refused."""
    cases = Z.refused_cases()
    for name, data, expected in cases:
        st = decode(cpu, data)[0]
        assert st == expected, (name, st)
        if expected == Z.CORRUPT:
            assert Z.pillow_pixels(data) is None, name
    names = {n for n, _, _ in cases}
    assert {"orientation_6", "unknown_tag", "exif_ifd", "xmp", "tiles", "lzw", "packbits", "uncompressed"} <= names


def test_the_three_probes_share_no_file(cpu, valid):
    """ke_parse_tiff, ke_parse_tiffc and ke_parse_tiffz over every tiff, tiffc and tiffz case file: no file is taken by two of
    them, and the new one takes nothing to which the uncompressed parser answers other than 1 -- what formats.files_offered
    rests on.  The first two answer the earlier modules' files as those modules' expectations say: the shared directory
    reading and second pass changed no status."""
    files = [d for _, d, _ in list(T.supported(True)) + list(T.handmade(True))] + [d for _, d, _ in T.refused()]
    files += [d for _, _, d in A.valid_cases()] + [d for _, d, _ in A.refused_cases()] + [d for _, d in A.late_change_cases()] + [d for _, d in A.damaged_set(40)]
    files += [d for _, _, d in valid] + [d for _, d, _ in Z.refused_cases()] + [d for _, d, _ in Z.corrupt_cases()] + Z.damaged_set(40)
    taken = Counter()
    for k, data in enumerate(files):
        st = (cpu.tiffz_cpu_probe_other(data, len(data), 0), cpu.tiffz_cpu_probe_other(data, len(data), 1), probe(cpu, data)[0])
        assert sum(s == 0 for s in st) <= 1, (k, st)
        assert st[2] != 0 or st[0] == 1, (k, st)
        for j, s in enumerate(st):
            taken[j] += s == 0
    assert all(taken[j] > 100 for j in range(3)), taken
    for _, name, data in A.valid_cases():
        assert (cpu.tiffz_cpu_probe_other(data, len(data), 0), cpu.tiffz_cpu_probe_other(data, len(data), 1)) == (1, 0), name
    for name, data, expected in A.refused_cases():
        if not name.startswith(("lzw_", "packbits_")):               # (those are refused by their streams, which no parser reads)
            assert cpu.tiffz_cpu_probe_other(data, len(data), 1) == expected, name
    for name, data, expected in T.refused():
        assert cpu.tiffz_cpu_probe_other(data, len(data), 0) == expected, name


def test_the_records_route_equals_the_plain_sink(cpu):
    """The kernels' way on the host: a strip through a sink that puts literals in place and writes matches down, the records
    then made in order byte by byte (length bias 3) -- the plane equals Pillow's, its Adler-32 summed by lanes equals the
    stream's trailer, and a strip has room for its records: at most one per 3 bytes it yields and one per 2 bits it has."""
    cases = Z.named_stream_cases() + Z.png_stream_cases()[::4] + [(n, d) for n, d in Z.handmade_cases() if "gray_" in n and "p2" not in n and "zero" not in n]
    copies = 0
    for name, data in cases:
        ref = Z.pillow_pixels(data)
        st, w, h, ch, comp, pred, nstrips, rows = probe(cpu, data)
        assert st == Z.OK and ch == 1, name
        regions = A._regions(data)[1]
        for s in range(nstrips):
            size = min(rows, h - s * rows) * w
            plane = np.zeros((size + 15) // 16 * 16 + 16, np.uint8)
            rec = np.zeros((size // 3 + 2, 2), np.uint32)
            n, want, trailer = C.c_uint32(), C.c_uint32(), C.c_uint32()
            assert cpu.tiffz_cpu_strip_records(data, len(data), s, plane.ctypes.data, rec.ctypes.data, C.byref(n), C.byref(want), C.byref(trailer)) == Z.OK, name
            assert want.value == size and n.value <= min(size // 3 + 2, regions[s][1] * 4 + 2), name
            flat = plane.tolist()
            for dst, word in rec[:n.value].tolist():
                for k in range((word & 511) + 3):
                    flat[dst + k] = flat[dst + k - (word >> 9)]
            plane[:] = flat
            copies += n.value
            assert np.array_equal(plane[:size], ref.ravel()[s * rows * w:s * rows * w + size]), name
            assert cpu.tiffz_cpu_adler_by_lanes(plane.ctypes.data, size) == trailer.value == zlib.adler32(plane[:size].tobytes()), name
    assert copies > 5000


def test_the_adler_sum_by_lanes_equals_zlib(cpu):
    """The sum as ke_tiffz_copies makes it, in 32-bit words, at the lengths at which a 32-bit sum first overflows (bytes of 0xFF:
    5 552 of them are the most zlib itself adds up between reductions), at every length up to 300 and on noise."""
    for n in (1, 5551, 5552, 5553, 65536, 1100000, 1 << 23):
        buf = np.full((n + 15) // 16 * 16, 255, np.uint8)
        assert cpu.tiffz_cpu_adler_by_lanes(buf.ctypes.data, n) == zlib.adler32(buf[:n].tobytes()), n
    rng = np.random.default_rng(8)
    noise = rng.integers(0, 256, 70000, dtype=np.uint8)
    for n in list(range(0, 300)) + [1023, 1024, 1025, 4097, 65521, 65537, 69999]:
        assert cpu.tiffz_cpu_adler_by_lanes(noise.ctypes.data, n) == zlib.adler32(noise[:n].tobytes()), n


def test_the_format_table_row(monkeypatch):
    """tiffz follows tiff at "hash" and "refine" and comes last at "refine_parallel"; absent with the variable unset and with
    KE_GPU_TIFF=0; with both TIFF opt-ins on, tiffc comes before tiffz."""
    sys.path.insert(0, ROOT)
    from kobato_eyes_amd import formats

    for v in ("KE_GPU_TIFF", "KE_GPU_TIFF_COMPRESSED", "KE_GPU_TIFF_DEFLATE", "KE_GPU_WEBP_LOSSLESS", "KE_GPU_WEBP_ALPHA", "KE_GPU_REFINE_DECODE"):
        monkeypatch.delenv(v, raising=False)
    kinds = lambda seam: [k for k, _ in formats.enabled_kinds(seam)]
    assert all("tiffz" not in kinds(seam) for seam in ("hash", "refine", "refine_parallel"))
    monkeypatch.setenv("KE_GPU_TIFF_DEFLATE", "1")
    for seam in ("hash", "refine"):
        assert kinds(seam)[kinds(seam).index("tiff") + 1] == "tiffz", seam
    assert kinds("refine_parallel")[-1] == "tiffz" and kinds("refine_parallel").index("tiff") < kinds("refine_parallel").index("webp")
    assert dict(formats.enabled_kinds("hash"))["tiffz"] == (".tif", ".tiff")
    assert formats.follow_ups("tiff") == ("tiffc", "tiffz") and "tiffz" not in formats.BASE_KINDS
    monkeypatch.setenv("KE_GPU_TIFF_COMPRESSED", "1")
    for seam in ("hash", "refine", "refine_parallel"):
        assert kinds(seam).index("tiffc") + 1 == kinds(seam).index("tiffz"), seam
    monkeypatch.setenv("KE_GPU_TIFF", "0")
    assert all("tiffz" not in kinds(seam) and "tiffc" not in kinds(seam) for seam in ("hash", "refine", "refine_parallel"))
    assert formats.files_offered("tiffz", ["a", "b", "c"], {"tiff": (["a", "b", "c"], [0, 1, 2])}) == ["b"]


def _fuzz(lib):
    census = Counter()
    for k, data in enumerate(Z.damaged_set()):
        st, out = decode(lib, data)
        assert st in (Z.OK, Z.UNSUPPORTED, Z.CORRUPT)
        ref = Z.pillow_pixels(data)
        census["cases"] += 1
        census["pillow"] += ref is not None
        if st == Z.OK:
            census["taken"] += 1
            assert ref is not None, f"damaged file {k} decoded where Pillow raises"
            assert out.shape == ref.shape and np.array_equal(out, ref), f"damaged file {k} decoded where Pillow differs"
    return census


def test_damage_fuzz(cpu):
    """2 400 damaged files (8 bases x 300: header and directory bytes, strip bits / bytes / stretches, bytes inserted, cuts, byte
    counts): status 0 => strict Pillow decodes the file to the same pixels (so Pillow raising => status != 0).  Both outcomes
    occur.  The floor comes from the damage itself: in each run of 16 files one has a single StripByteCounts value moved by
    -6 .. +6 (tests/_tiffc_cases.damaged, k % 16 == 6), 19 per base and 152 in all, of which a fifth is overwritten by the
    insertions; for 7 of the 13 amounts (0 .. +6) every strip is still a whole stream, followed by bytes that are ignored, so
    about 65 files must be taken.  Asserted: half of that, 32 -- refusing everything does not pass.  The census is printed."""
    census = _fuzz(cpu)
    print(f"damage census: {census['cases']} cases, Pillow takes {census['pillow']}, the decoder takes {census['taken']}")
    assert census["cases"] == 2400
    assert census["taken"] >= 32 and 0 < census["pillow"] < census["cases"]


def test_sanitised_build(tmp_path_factory):
    """The host code under AddressSanitizer and UBSan, as a program of its own: the valid hand-made sets, the refusals, the odd
    strips and 800 mutations -- statuses and pixels as Pillow's, the Adler sum by lanes equal to the sequential one, no report."""
    cxx = _cxx()
    work = tmp_path_factory.mktemp("tiffz_san")
    exe = str(work / "tiffz_san")
    base = [cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKE_TIFFZ_MAIN", "-I", CSRC,
            os.path.join(ROOT, "tests", "_tiffz_cpu.cpp"), "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    rng = np.random.default_rng(98)
    files = [(n, d, e) for n, d, e in Z.refused_cases()] + [(n, d, e) for n, d, e, _ in Z.odd_strip_cases()]
    files += [(n, d, Z.OK) for n, d in Z.named_stream_cases() + Z.png_stream_cases() + Z.handmade_cases()]
    files += [(f"mutation_{k}", d, None) for b in Z.fuzz_bases() for k, d in enumerate(Z.damaged(b, rng, 100))]
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
        st, w, h, ch, same = (int(v) for v in line.split())
        assert same == 1, name
        if expected is not None:
            assert st == expected, name
        if st == Z.OK:
            ref = Z.pillow_pixels(data)
            shape = (h, w) if ch == 1 else (h, w, ch)
            assert ref is not None and ref.shape == shape, name
            assert np.array_equal(np.fromfile(path + ".out", np.uint8).reshape(shape), ref), name
            taken += expected is None
    print(f"sanitised build: {len(files)} files, {taken} mutations taken")
    assert len(files) >= 800 + 300
