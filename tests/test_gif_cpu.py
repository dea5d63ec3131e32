"""The product's GIF container walk and LZW arithmetic (csrc/ke_gif_core.h, the header ke_gif.hip compiles) built for the host
(oracle/libkeyes_gif_cpu.so) against the installed Pillow: the first frame's luma, pixel-exact, for every file the decoder takes;
a refusal for the rest; under random damage never a file taken that Pillow refuses or shows differently.

Hand-written code streams (tests/_gif_write.py, tests/_gif_stream_cases.py): 250 valid ones (177 stream features counted by the
writer, 86 features of the copy records counted from the records the kernels' own sink makes -- csrc/ke_lz_records.h -- 24 013
records in 133 runs among them, the longest run of each distance 2..16: 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9 copies), 65
invalid ones (53 with status 2, 12 with status 1), 1 000 random ones (135 216 records, 1 364 runs in all three sets).  Each is
decoded directly and through the sink with the records replayed in order.  The decoder refuses no stream that Pillow takes.
What the issue's list asked for and LZW cannot produce -- runs of 70 copies, phases 1, strings above 513 inside 128 x 128
pixels -- is stated in tests/_gif_stream_cases.py and asserted by test_what_lzw_cannot_record."""
from __future__ import annotations

import ctypes as C
import functools
import os
import shutil
import subprocess
import zlib
from collections import Counter

import numpy as np
import pytest
from PIL import ImageFile

import _gif_cases as G
import _gif_stream_cases as S
from oracle import oracle as O


def _lib():
    here = os.path.dirname(O.__file__)
    path = os.path.join(here, "libkeyes_gif_cpu.so")
    subprocess.check_call(["make", "-C", here, "-s", "libkeyes_gif_cpu.so"])      # before the first load: make knows whether it is stale
    L = C.CDLL(path)
    L.ko_gif_records.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ko_gif_replay.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.ko_gif_probe.argtypes = [C.c_void_p, C.c_uint64] + [C.POINTER(C.c_int32)] * 3
    L.ko_gif_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def _decode(L, data: bytes):
    buf = np.frombuffer(data + b"\0", np.uint8)
    w, h, ch = C.c_int32(), C.c_int32(), C.c_int32()
    st = L.ko_gif_probe(buf.ctypes.data, len(data), C.byref(w), C.byref(h), C.byref(ch))
    if st:
        return st, None
    out = np.empty((h.value, w.value), np.uint8)
    st = L.ko_gif_decode(buf.ctypes.data, len(data), out.ctypes.data)
    return st, (out if st == 0 else None)


def strict_pillow(data: bytes):
    saved, ImageFile.LOAD_TRUNCATED_IMAGES = ImageFile.LOAD_TRUNCATED_IMAGES, False
    try:
        return G._pillow(data)
    except Exception:
        return None
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = saved


def test_first_frame_matches_pillow():
    L = _lib()
    n = 0
    for name, data, ref in list(G.supported()) + list(G.handmade()):
        st, out = _decode(L, data)
        if ref is None or name.startswith(G.LEFT_TO_PILLOW):
            assert st != 0, name
            continue
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name
        n += 1
    assert n > 120


def test_files_outside_the_decoder_are_refused():
    L = _lib()
    for name, data, expected in G.refused():
        st, _ = _decode(L, data)
        assert st == expected, name
        if expected == 2:
            assert strict_pillow(data) is None, name


def damaged(rng, pool, variants):
    for name, data, _ in pool:
        for v in range(variants):
            d = bytearray(data)
            how = v % 5
            if how == 0:
                pos = int(rng.integers(6, len(d)))
                d[pos] = int(rng.integers(0, 256))
            elif how == 1:
                pos = int(rng.integers(6, len(d)))
                d[pos] ^= 1 << int(rng.integers(0, 8))
            elif how == 2:
                d = d[: int(rng.integers(13, len(d)))]
            elif how == 3:
                pos = int(rng.integers(6, len(d)))
                del d[pos:pos + int(rng.integers(1, 5))]
            else:
                pos = int(rng.integers(6, len(d)))
                d[pos:pos] = rng.integers(0, 256, int(rng.integers(1, 5)), dtype=np.uint8).tobytes()
            yield f"{name}/{v}", bytes(d)


def test_damaged_files_are_never_decoded_differently_from_pillow():
    L = _lib()
    rng = np.random.default_rng(33)
    pool = [c for c in list(G.supported()) + list(G.handmade()) if c[2] is not None and c[2].size <= 8000]
    taken = cases = 0
    for name, data in damaged(rng, pool, 30):
        cases += 1
        st, out = _decode(L, data)
        if st != 0:
            continue
        taken += 1
        ref = strict_pillow(data)
        assert ref is not None, name
        assert ref.shape == out.shape and np.array_equal(ref, out), name
    assert cases > 2000 and taken > 200


# ---- hand-written code streams (tests/_gif_write.py, tests/_gif_stream_cases.py) ---------------------------------------------------
def hold_to_pillow(cases, decode):
    """cases: (name, file, Pillow's luma or None, census or the expected status); decode(file) -> (status, pixels).  Status 0:
    Pillow opens the file, with equal pixels; 2: Pillow raises; 1 only where the case names it."""
    failures = []
    for name, data, ref, expected in cases:
        expected = expected if isinstance(expected, int) else 0
        st, out = decode(data)
        if st != expected:
            failures.append(f"{name}: status {st}, expected {expected}")
        elif st == 0 and (ref is None or out.shape != ref.shape or not np.array_equal(out, ref)):
            failures.append(f"{name}: {'Pillow refuses the file' if ref is None else 'pixels differ from those of Pillow'}")
        elif st == 2 and ref is not None:
            failures.append(f"{name}: status 2, but Pillow takes the file")
    return failures


def all_streams():
    return list(S.valid()) + list(S.invalid()) + list(S.random_streams())


def test_hand_written_streams_decode_as_pillow_does():
    L = _lib()
    failures = hold_to_pillow(S.valid(), lambda d: _decode(L, d))
    assert not failures, failures[:10]
    assert len(S.valid()) >= 200


def test_the_valid_set_holds_every_feature_it_is_there_for():
    """The census of what the writer wrote (counted by the writer) against the list of features the set exists for."""
    census = sum((c[3] for c in S.valid()), Counter())
    missing = [f for f in S.valid_features() if not census[f]]
    assert not missing, missing
    assert census["codes_with_a_full_table_bits_2"] >= 500 and all(census[f"codes_with_a_full_table_bits_{b}"] >= 500 for b in range(2, 9))
    assert len(S.valid_features()) > 160


def test_invalid_streams_get_the_status_their_rule_names():
    L = _lib()
    failures = hold_to_pillow(S.invalid(), lambda d: _decode(L, d))
    assert not failures, failures[:10]
    assert len(S.invalid()) >= 60 and sum(1 for c in S.invalid() if c[3] == 2) >= 50


def test_random_streams_decode_as_pillow_does():
    L = _lib()
    failures = hold_to_pillow(S.random_streams(), lambda d: _decode(L, d))
    assert not failures, failures[:10]
    assert len(S.random_streams()) == S.RANDOM_STREAMS == 1000


def records_of(L, data: bytes):
    """(status, records n x 2, the indices with the literals in place, width x height) through the kernels' sink."""
    buf = np.frombuffer(data + b"\0", np.uint8)
    w, h, ch = C.c_int32(), C.c_int32(), C.c_int32()
    if L.ko_gif_probe(buf.ctypes.data, len(data), C.byref(w), C.byref(h), C.byref(ch)):
        return None
    want = w.value * h.value
    idx = np.zeros(want + 2, np.uint8)
    rec = np.zeros((want // 2 + 2, 2), np.uint32)                     # the bound the kernel's scratch rests on
    n = C.c_uint32()
    st = L.ko_gif_records(buf.ctypes.data, len(data), idx.ctypes.data, rec.ctypes.data, C.byref(n))
    return st, rec[:n.value], idx, (h.value, w.value)


@functools.lru_cache(None)
def record_census():
    """Per stream of the three sets: (name, status, census of its records), the replayed pixels checked on the way."""
    L = _lib()
    out = []
    for name, data, ref, _ in all_streams():
        got = records_of(L, data)
        if got is None:
            out.append((name, -1, Counter(), None))
            continue
        st, rec, idx, shape = got
        pixels = None
        if st == 0:
            pixels = np.empty(shape, np.uint8)
            buf = np.frombuffer(data + b"\0", np.uint8)
            assert L.ko_gif_replay(buf.ctypes.data, len(data), idx.ctypes.data, rec.ctypes.data, len(rec), pixels.ctypes.data) == 0, name
        out.append((name, st, S.records_census(rec, shape[0] * shape[1]) + Counter(records=len(rec), pixels=shape[0] * shape[1]), pixels))
    return out


def test_replayed_records_equal_the_direct_decode_and_pillow():
    """The kernels' way on the host: the code stream through the shared sink (csrc/ke_lz_records.h), the recorded copies made
    strictly in order byte by byte -- the same status as the direct decode for every stream, and for every stream taken the
    same pixels, which are Pillow's."""
    L = _lib()
    taken = 0
    for (name, data, ref, _), (_, st, _, pixels) in zip(all_streams(), record_census()):
        direct, out = _decode(L, data)
        assert st == direct, name
        if st == 0:
            taken += 1
            assert np.array_equal(pixels, out) and ref is not None and np.array_equal(pixels, ref), name
    assert taken >= len(S.valid()) + S.RANDOM_STREAMS


def test_the_record_count_stays_within_the_kernels_scratch():
    """nrec <= width * height / 2 + 2 (ke_gif.hip sizes the records by it) for every stream, refused ones too."""
    for name, st, census, _ in record_census():
        assert census["records"] <= census["pixels"] // 2 + 2, name
    assert max(c["records"] * 2 / max(c["pixels"], 1) for _, _, c, _ in record_census() if c["pixels"] >= 16) > 0.6


def test_the_records_of_the_valid_set_hold_every_copy_pattern():
    """Counted from the product's own records: piece lengths, pieces of one string, runs of every distance 2..16 at their
    longest and across a round of 64, phases, a blocker in front of a run, distance 17, distance 1, a dependent chain."""
    names = {c[0] for c in S.valid()}
    census = sum((c for name, _, c, _ in record_census() if name in names), Counter())
    missing = [f for f in S.record_features() if not census[f]]
    assert not missing, missing


def test_what_lzw_cannot_record():
    """See tests/_gif_stream_cases.py: in no stream of the three sets does a copy of a run other than its last begin d or more
    pixels behind the run's head, no run has distance 1, no phase is 1, and no piece is longer than 17 at a distance up to
    16 -- which is why the sets do not ask for runs of 70 copies."""
    runs = 0
    for name, _, c, _ in record_census():
        runs += c["runs"]
        assert not c["runs_with_a_source_behind_the_head"], name
        assert not any(k.startswith("run_d1_") or (k.startswith("run_d") and k.endswith("_phase_1")) for k in c), name
        assert all(int(k.split("_")[1][1:]) // 2 + 1 >= int(k.split("_")[3]) for k in c if k.startswith("run_d") and "_of_" in k), name
    assert runs >= 100


def test_sanitised_streams_build(tmp_path_factory):
    """The host build under AddressSanitizer and UBSan, as a program of its own (the sanitiser's runtime linked in): the three
    sets, each stream decoded directly and through the sink and the replay, with buffers of exactly the sizes the kernels
    reserve -- statuses and pixels as the plain build's, and no report."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    work = tmp_path_factory.mktemp("gif_san")
    exe = str(work / "gif_san")
    base = [cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            os.path.join(root, "tests", "_gif_san_main.cpp"), "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    L = _lib()
    cases = all_streams()
    paths = []
    for k, c in enumerate(cases):
        paths.append(str(work / f"{k}.gif"))
        with open(paths[-1], "wb") as f:
            f.write(c[1])
    with open(work / "list.txt", "w") as f:
        f.write("\n".join(paths) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")
    res = subprocess.run([exe, str(work / "list.txt")], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        st, out = _decode(L, c[1])
        sum_ = zlib.adler32(out.tobytes()) if st == 0 else 1
        assert line == f"{st} {sum_} {st} {sum_}", c[0]
