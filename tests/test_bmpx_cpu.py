"""The host parse of the decoder for RLE, 1 / 4-bit and 16-bit BMP files and the arithmetic its kernels run (ke_bmpx_parse.h,
ke_bmpx_core.h, and ke_bmp_parse.h's header reader they share with ke_parse_bmp) compiled for the CPU and held against Pillow's
BmpImagePlugin, bit for bit: every valid file taken with Pillow's shape and bytes, the refusals with their status and, where
Pillow opens the file, by name; the rule over every file of every set; the records route; every file cut at every length (the six
131 KB files of all 16-bit values at a stated sample of lengths) and
single-byte changes; ke_parse_bmp and ke_parse_bmpx against each other; the format table's row; a sanitised program of its own.
No GPU needed: the headers are compiled with the host C++ compiler (tests/_bmpx_cpu.cpp) into a temporary directory."""
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
import _bmp_cases as B  # noqa: E402
import _bmpx_cases as X  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bmpx_cpu") / "bmpx_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-shared", "-fPIC", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "_bmpx_cpu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.bmpx_cpu_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.bmpx_cpu_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.bmpx_cpu_probe_bmp.argtypes = [C.c_char_p, C.c_uint64]
    lib.bmpx_cpu_records.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    return lib


def probe(lib, data: bytes):
    """status, width, height, channels, kind, topdown, data offset, stride"""
    info = np.zeros(8, np.int32)
    lib.bmpx_cpu_probe(data, len(data), info.ctypes.data)
    return tuple(int(v) for v in info)


def decode(lib, data: bytes):
    st, w, h, ch = probe(lib, data)[:4]
    if st != X.OK:
        return st, None
    out = np.zeros((h, w) if ch == 1 else (h, w, ch), np.uint8)
    st = lib.bmpx_cpu_decode(data, len(data), out.ctypes.data)
    return st, out


def named_refusal(name: str):
    return next((k for k in X.NAMED_REFUSALS if name.startswith(k)), None)


def test_every_valid_file_equals_pillow(cpu):
    census = Counter()
    for name, data, features in X.valid_cases():
        ref = X.pillow_pixels(data)
        assert ref is not None, name
        st, out = decode(cpu, data)
        assert st == X.OK, (name, st)
        assert out.shape == ref.shape, (name, out.shape, ref.shape)
        assert np.array_equal(out, ref), name
        census.update(features)
    print("features:", dict(census))
    missing = [f for f in X.FEATURES if census[f] == 0]
    assert not missing, missing
    assert all(census[f"grid_{k}"] == 60 for k in X.KINDS) and all(census[f"every_value_{k}"] == 2 for k in ("rgb555", "rgb555m", "rgb565"))
    assert census["real_picture"] >= 12


def test_what_the_issue_states_about_pillow(cpu):
    """The claims the decoder was written from, re-checked against the installed Pillow rather than trusted."""
    by_name = {n: d for n, d, _ in X.valid_cases()}
    assert X.pillow_pixels(by_name["rle8_example_rows_1234_7777"]).tolist() == [[1, 2, 3, 4], [7, 7, 7, 7]]
    px = np.array([[0x1234]], np.uint16)
    assert X.pillow_pixels(X.picture("rgb555", px)).tolist() == [[[32, 139, 164]]] == decode(cpu, X.picture("rgb555", px))[1].tolist()
    assert X.pillow_pixels(X.picture("rgb565", px)).tolist() == [[[16, 68, 164]]] == decode(cpu, X.picture("rgb565", px))[1].tolist()
    bw = X.pillow_pixels(by_name["p1_black_white_9x3"])
    assert set(np.unique(bw).tolist()) <= {0, 255}
    # RLE4 absolute of an odd n: n - 1 pixels, and the run behind it is cut as if n had been written
    odd = X.pillow_pixels(by_name["rle4_absolute_every_n_5"])
    even = X.pillow_pixels(by_name["rle4_absolute_every_n_4"])
    assert odd is not None and even is not None and not np.array_equal(odd, even)


def test_every_invalid_file_has_its_status(cpu):
    """The status per file.  Pillow raises on open or load -- or the case is a refusal listed by name with its reason."""
    named = set()
    cases = X.invalid_cases()
    for name, data, expected in cases:
        st, _ = decode(cpu, data)
        assert st == expected, (name, st)
        if X.pillow_pixels(data) is not None:
            key = named_refusal(name)
            assert expected == X.UNSUPPORTED and key is not None, f"{name}: Pillow opens it, and no named refusal covers it"
            named.add(key)
    assert named == set(X.NAMED_REFUSALS), sorted(named ^ set(X.NAMED_REFUSALS))
    names = {n for n, _, _ in cases}
    for t in ("rle8", "rle4"):
        assert {f"{t}_early_end_of_bitmap", f"{t}_cut_after_one_byte_of_a_code", f"{t}_cut_inside_an_absolute_payload", f"{t}_cut_inside_a_delta",
                f"{t}_pixels_short_by_one"} <= names
    assert {"p4_pixel_data_short_by_one", "unknown_16_bit_masks_0_hs40", "compression_4", "compression_5", "rle_with_24_bits",
            "colors_above_256_at_4_bits"} <= names


def _hold_to_the_rule(cpu, name, data, census):
    """status 0 => Pillow takes the file with equal pixels; Pillow takes it => status 0, or a named refusal."""
    st, out = decode(cpu, data)
    assert st in (X.OK, X.UNSUPPORTED, X.CORRUPT), (name, st)
    ref = X.pillow_pixels(data)
    census["files"] += 1
    census["pillow"] += ref is not None
    if st == X.OK:
        census["taken"] += 1
        assert ref is not None, f"{name}: decoded where Pillow raises"
        assert out.shape == ref.shape and np.array_equal(out, ref), f"{name}: decoded where Pillow differs"
    return st, ref


def test_the_rule_over_every_file_of_every_set(cpu):
    census = Counter()
    for name, data in X.every_file():
        st, ref = _hold_to_the_rule(cpu, name, data, census)
        if ref is not None and st != X.OK:
            assert st == X.UNSUPPORTED and named_refusal(name) is not None, (name, st)
    random = Counter(decode(cpu, d)[0] for _, d in X.random_cases())
    print("every set:", dict(census), "random streams by status:", dict(random))
    assert len(X.random_cases()) == 1000 and random[X.OK] >= 500 and random[X.CORRUPT] >= 50 and random[X.UNSUPPORTED] == 0


def test_the_records_route(cpu):
    """ke_bmpx_codes' records from the host build, replayed byte by byte here: every record inside [0, W * H), at most one per
    two bytes of the stream, and the picture they give -- over a plane cleared to index 0 -- is Pillow's."""
    files = [(n, d) for n, d, _ in X.valid_cases() if n.startswith(("rle8", "rle4"))] + list(X.random_cases()[:300])
    records = literals = 0
    for name, data in files:
        st, w, h, ch, kind, topdown, off, _ = probe(cpu, data)
        if st != X.OK:                                       # a file without a single byte of stream
            assert st == X.CORRUPT and off == 0 and X.pillow_pixels(data) is None, name
            continue
        cap = (len(data) - off) // 2
        rec = np.zeros((cap + 1, 4), np.uint32)
        n, lut = C.c_uint32(), np.zeros(256, np.uint8)
        st = cpu.bmpx_cpu_records(data, len(data), rec.ctypes.data, cap, C.byref(n), lut.ctypes.data)
        assert n.value <= cap, name
        ref = X.pillow_pixels(data)
        assert (st == X.OK) == (ref is not None), name
        if st != X.OK:
            continue
        stream, rle4 = data[off:], kind == 2
        flat = [0] * (w * h)
        for pos, length, literal, arg in rec[:n.value].tolist():
            assert 0 <= pos and length >= 1 and pos + length <= w * h, (name, pos, length)
            for k in range(length):
                if literal:
                    v = stream[arg + (k >> 1)] if rle4 else stream[arg + k]
                    v = (v & 15 if k & 1 else v >> 4) if rle4 else v
                else:
                    v = (arg & 15 if k & 1 else arg >> 4) if rle4 else arg
                flat[pos + k] = v
            literals += literal
        records += n.value
        got = lut[np.array(flat, np.int64).reshape(h, w)]
        assert np.array_equal(got if topdown else got[::-1], ref), name
    assert records > 5000 and literals > 500


def _cuts(data: bytes, probe_info) -> list:
    """The lengths a valid file is cut at: every one -- except for the six files of all 65 536 16-bit values (131 KB each, 256 stored
    rows of 512 bytes), which are cut at a stated sample: every length through the header and the first two stored rows, the five
    lengths around every boundary between stored rows, and every length of the last stored row."""
    if len(data) <= 20000:
        return list(range(len(data)))
    off, stride = probe_info[6], probe_info[7]
    cuts = set(range(0, off + 2 * stride + 1)) | set(range(len(data) - stride - 2, len(data)))
    for row in range(2, (len(data) - off) // stride + 1):
        cuts |= set(range(off + row * stride - 2, off + row * stride + 3))
    return sorted(c for c in cuts if 0 <= c < len(data))


def test_every_valid_file_cut_at_every_length(cpu):
    """Every valid case cut at every length (the six 131 KB files at the sample ``_cuts`` states): the rule holds for each cut."""
    census, sampled = Counter(), []
    for name, data, _ in X.valid_cases():
        cuts = _cuts(data, probe(cpu, data))
        if len(cuts) < len(data):
            sampled.append(name)
        for cut in cuts:
            _hold_to_the_rule(cpu, f"{name}[:{cut}]", data[:cut], census)
    print("cuts:", dict(census), "sampled:", sampled)
    assert sorted(sampled) == sorted(n for n, _, _ in X.valid_cases() if "every_value" in n) and len(sampled) == 6
    assert census["files"] > 240000 and 0 < census["taken"] < census["files"]


def test_single_byte_changes(cpu):
    census = Counter()
    for name, data in X.byte_changes():
        _hold_to_the_rule(cpu, name, data, census)
    print("byte changes:", dict(census))
    assert census["files"] == 2000 and census["taken"] >= 200 and census["pillow"] < census["files"]


def test_bmp_and_bmpx_share_no_file(cpu):
    """ke_parse_bmp and ke_parse_bmpx over every bmp and bmpx case file: no file is taken by both, and the new one takes nothing
    to which ke_parse_bmp answers other than 1 -- what formats.files_offered rests on.  ke_parse_bmp still answers its own
    module's refusals as that module says."""
    files = [d for _, d, _ in list(B.supported()) + list(B.handmade())] + [d for _, d, _ in B.refused()] + [d for _, d in X.every_file()]
    files += [d for _, d in X.byte_changes(600)]
    taken = Counter()
    for k, data in enumerate(files):
        st = (cpu.bmpx_cpu_probe_bmp(data, len(data)), probe(cpu, data)[0])
        assert st != (0, 0) and (st[1] != 0 or st[0] == 1), (k, st)
        taken.update(j for j in (0, 1) if st[j] == 0)
    assert taken[0] > 100 and taken[1] > 1000, taken
    for name, data, expected in B.refused():
        assert cpu.bmpx_cpu_probe_bmp(data, len(data)) == expected, name


def test_a_damaged_depth_field_is_not_shifted_by(cpu):
    """The shared reader computes 1 << bits only for a depth that has a palette (the sanitised build below runs the same files)."""
    base = bytearray(X.picture("rgb555", np.zeros((2, 2), np.uint16)))
    for bits in (64, 255, 4096, 65535):
        base[28:30] = bits.to_bytes(2, "little")
        assert probe(cpu, bytes(base))[0] == X.UNSUPPORTED and cpu.bmpx_cpu_probe_bmp(bytes(base), len(base)) == 1


def test_the_format_table_row(monkeypatch):
    """bmpx follows bmp at "hash" and "refine" and comes behind the base kinds at "refine_parallel"; absent with the variable
    unset and with KE_GPU_BMP=0."""
    sys.path.insert(0, ROOT)
    from kobato_eyes_amd import formats

    for v in ("KE_GPU_BMP", "KE_GPU_BMP_EXTENDED", "KE_GPU_TIFF", "KE_GPU_TIFF_COMPRESSED", "KE_GPU_TIFF_DEFLATE", "KE_GPU_WEBP_LOSSLESS",
              "KE_GPU_WEBP_ALPHA", "KE_GPU_REFINE_DECODE"):
        monkeypatch.delenv(v, raising=False)
    kinds = lambda seam: [k for k, _ in formats.enabled_kinds(seam)]
    assert all("bmpx" not in kinds(seam) for seam in ("hash", "refine", "refine_parallel"))
    monkeypatch.setenv("KE_GPU_BMP_EXTENDED", "1")
    assert kinds("hash") == ["jpeg", "png", "bmp", "bmpx", "gif", "tiff", "webp"]
    assert kinds("refine") == ["jpeg", "png", "bmp", "bmpx", "tiff", "webp"]
    assert kinds("refine_parallel") == ["jpeg", "png", "bmp", "gif", "tiff", "webp", "bmpx"]
    assert dict(formats.enabled_kinds("hash"))["bmpx"] == (".bmp",)
    assert formats.follow_ups("bmp") == ("bmpx",) and "bmpx" not in formats.BASE_KINDS and "bmpx" in formats.KINDS
    monkeypatch.setenv("KE_GPU_TIFF_DEFLATE", "1")
    assert kinds("refine_parallel")[-2:] == ["bmpx", "tiffz"]
    monkeypatch.setenv("KE_GPU_BMP", "0")
    assert all("bmpx" not in kinds(seam) and "bmp" not in kinds(seam) for seam in ("hash", "refine", "refine_parallel"))
    assert formats.files_offered("bmpx", ["a", "b", "c"], {"bmp": (["a", "b", "c"], [0, 1, 2])}) == ["b"]


def test_sanitised_build(tmp_path_factory):
    """The host code under AddressSanitizer and UBSan, as a program of its own that reads the files from a directory: every valid,
    invalid and random case, 2 000 byte changes, cuts (the bases at every third length, the two longest real RLE8 streams at every
    length), and headers with a damaged depth -- statuses and pixels as Pillow's, no report."""
    cxx = _cxx()
    work = tmp_path_factory.mktemp("bmpx_san")
    exe = str(work / "bmpx_san")
    base = [cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DKE_BMPX_MAIN", "-I", CSRC,
            os.path.join(ROOT, "tests", "_bmpx_cpu.cpp"), "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    files = [(n, d, X.OK) for n, d, _ in X.valid_cases()] + list(X.invalid_cases()) + [(n, d, None) for n, d in X.random_cases()]
    files += [(n, d, None) for n, d in X.byte_changes()]
    for name, data in X.fuzz_bases():
        files += [(f"{name}[:{cut}]", data[:cut], None) for cut in range(0, min(len(data), 1300), 3)]
    by_name = {n: d for n, d, _ in X.valid_cases()}
    for name in ("rle8_picture_smooth_1", "rle8_picture_noise_2"):          # the longest real streams, at every length
        files += [(f"{name}[:{cut}]", by_name[name][:cut], None) for cut in range(len(by_name[name]))]
    damaged = bytearray(X.picture("rgb555", np.zeros((2, 2), np.uint16)))
    for bits in (64, 255, 4096, 65535):
        damaged[28:30] = bits.to_bytes(2, "little")
        files.append((f"depth_{bits}", bytes(damaged), X.UNSUPPORTED))
    paths = []
    for k, (_, data, _) in enumerate(files):
        paths.append(str(work / f"{k}.bmp"))
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
        if st == X.OK:
            ref = X.pillow_pixels(data)
            shape = (h, w) if ch == 1 else (h, w, ch)
            assert ref is not None and ref.shape == shape, name
            assert np.array_equal(np.fromfile(path + ".out", np.uint8).reshape(shape), ref), name
            taken += expected is None
    print(f"sanitised build: {len(files)} files, {taken} of the damaged and random ones taken")
    assert len(files) >= 5000 and taken >= 500
