"""The product's PNG arithmetic (csrc/ke_png_core.h + ke_png_parse.h, the headers the HIP kernels compile) built for the host
(oracle/libkeyes_png_cpu.so) against the installed Pillow: pixel-exact on every file the decoder takes, the right refusal for
the rest.  The GPU kernels are then held against Pillow directly (tests/test_gpu_jpeg.py)."""
from __future__ import annotations

import ctypes as C
import functools
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import _png_cases as P
from oracle import oracle as O


def _lib():
    path = os.path.join(os.path.dirname(O.__file__), "libkeyes_png_cpu.so")
    if not os.path.exists(path):
        O.build(force=True)
    L = C.CDLL(path)
    L.ko_png_probe.argtypes = [C.c_void_p, C.c_uint64] + [C.POINTER(C.c_int32)] * 3
    L.ko_png_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def _decode(L, data: bytes):
    buf = np.frombuffer(data + b"\0", np.uint8)
    w, h, ch = C.c_int32(), C.c_int32(), C.c_int32()
    st = L.ko_png_probe(buf.ctypes.data, len(data), C.byref(w), C.byref(h), C.byref(ch))
    if st:
        return st, None
    out = np.empty((h.value, w.value, ch.value) if ch.value > 1 else (h.value, w.value), np.uint8)
    return L.ko_png_decode(buf.ctypes.data, len(data), out.ctypes.data), out


def test_decoder_arithmetic_matches_pillow():
    L = _lib()
    n = 0
    for name, data, ref in list(P.supported()) + list(P.handmade()) + list(P.mapped()) + list(P.interlaced()) + list(P.wide()):
        st, out = _decode(L, data)
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name
        n += 1
    assert n > 100


def test_damaged_files_the_decoder_takes_are_decoded_as_pillow_does():
    """tests/fuzz_jpeg_damage.py --png, a bounded sample: bytes changed, flipped, deleted, inserted anywhere behind the
    signature, truncation.  Nearly everything is refused (chunk checksums, the zlib checksum); what is taken has Pillow's
    pixels, and Pillow takes it too."""
    import fuzz_jpeg_damage as F

    cases, taken, wrong = F.check(F.cpu_decoder("png"), 25, 3, files=40, fmt="png")
    assert not wrong, wrong[:5]
    assert cases == 2000 and taken >= 1


def test_files_outside_the_decoder_are_refused():
    L = _lib()
    for name, data, expected in P.refused():
        st, _ = _decode(L, data)
        assert st == expected, name


def test_random_files_decode_as_pillow_does():
    """Property: whatever 8-bit image Pillow writes as a non-interlaced PNG -- any size up to 80 x 60, L / RGB / RGBA / P /
    bilevel, any compression level, optimised or not, with transparency for palette files -- the decoder arithmetic yields what
    the reference's hashes see (the pixels, or convert("L") of them for the mapped kinds)."""
    import io

    from hypothesis import given, settings
    from hypothesis import strategies as st
    from PIL import Image

    L = _lib()

    @settings(max_examples=120, deadline=None, derandomize=True)
    @given(st.integers(1, 80), st.integers(1, 60), st.sampled_from(["L", "RGB", "RGBA", "P", "1"]), st.integers(0, 9), st.booleans(),
           st.integers(0, 3), st.integers(0, 2 ** 32 - 1))
    def check(w, h, mode, level, optimize, texture, seed):
        rng = np.random.default_rng(seed)
        if texture == 0:
            a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        elif texture == 1:
            a = np.repeat(np.repeat(rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 4), dtype=np.uint8), 8, 0), 8, 1)[:h, :w]
        elif texture == 2:
            a = np.broadcast_to(rng.integers(0, 256, (1, 1, 4), dtype=np.uint8), (h, w, 4)).copy()
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            a = np.stack([xx * 3 % 256, yy * 5 % 256, (xx + yy) % 256, (xx * yy) % 256], -1).astype(np.uint8)
        if mode == "P":
            im = Image.fromarray(a[:, :, :3]).quantize(int(rng.integers(2, 257)))
        elif mode == "1":
            im = Image.fromarray(a[:, :, 0]).convert("1")
        else:
            im = Image.fromarray({"L": a[:, :, 0], "RGB": a[:, :, :3], "RGBA": a}[mode])
        kw = {"compress_level": level, "optimize": optimize}
        if mode == "P" and seed & 1:
            kw["transparency"] = int(seed >> 8) % 2
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        data = b.getvalue()
        with Image.open(io.BytesIO(data)) as back:
            ref = np.asarray(back.convert("L") if back.mode in ("P", "1") else back)
        status, out = _decode(L, data)
        assert status == 0 and out.shape == ref.shape and np.array_equal(out, ref)

    check()


def test_random_handmade_files_decode_as_pillow_does():
    """What Pillow's writer never produces -- interlacing, 16 bits, sub-byte grayscale, short palettes, every filter type in any
    row, IDAT data in chunks of a few bytes -- in random combinations (tests/_png_cases.random_handmade)."""
    L = _lib()
    n = 0
    for name, data, ref in P.random_handmade(400, 17):
        st, out = _decode(L, data)
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name
        n += 1
    assert n == 400


def test_animated_files_yield_frame_0():
    """Animated PNG: what Image.open shows is frame 0 -- the IDAT image; files in forms the parser does not mirror are refused
    (and whatever it takes is what Pillow shows, also when Pillow itself refuses the hand-edited file: then it must not be taken)."""
    import io

    from PIL import Image

    L = _lib()
    n = 0
    for name, data, ref in P.animated():
        st, out = _decode(L, data)
        if ref is None:
            assert st != 0, name
            continue
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name
        n += 1
    assert n >= 30


# ---- hand-written deflate streams (tests/_deflate_write.py, the generators in tests/_png_cases.py) -----------------------------
RANDOM_BLOCK_LISTS = 1000        # (1 000 take 24 s to write, judge and decode on the host, 2 000 take 50 s; the feature list is not cut)

# deflate_invalid cases the decoder refuses and Pillow takes -- the only asymmetry allowed: (IDAT chunkings, reason).  Pillow
# hands zlib the data chunk by chunk and stops once the last row is there; what lies in a chunk it never hands on is not seen.
_ALL = ("idat_1", "idat_7", "idat_whole")
_STRICTER = {
    "adler_wrong_in_the_last_byte": (_ALL[:2], "the decoder holds the Adler-32; Pillow has its last row before the chunk with the trailer"),
    "adler_wrong_in_the_first_byte": (_ALL[:2], "as above"),
    "literal_one_byte_past_the_image": (_ALL, "a stream that inflates to more than the image is refused; Pillow stops at the last row"),
    "copy_one_byte_past_the_image": (_ALL, "as above, the byte too many comes from a copy"),
    "stored_block_one_byte_past_the_image": (_ALL, "as above, from a stored block"),
    "damaged_block_behind_the_image": (_ALL[:1], "the decoder reads the stream to its end; Pillow has its last row before that chunk"),
    "stream_ends_1_bytes_short": (_ALL, "the Adler-32 is cut: the decoder wants all four bytes, Pillow never asks for them"),
    "stream_ends_2_bytes_short": (_ALL, "as above"),
    "stream_ends_4_bytes_short": (_ALL, "as above, the whole Adler-32 is missing"),
    "stream_ends_5_bytes_short": (_ALL, "the end-of-block code of the final block is cut; Pillow has its last row by then"),
    "stream_without_a_final_block": (_ALL, "the stream goes on behind the image; Pillow has its last row by then"),
}
STRICTER_THAN_PILLOW = {f"{stem}_{tag}": why for stem, (tags, why) in _STRICTER.items() for tag in tags}


@functools.lru_cache(None)
def valid_cases():
    return tuple(P.deflate_valid())


@functools.lru_cache(None)
def invalid_cases():
    return tuple(P.deflate_invalid())


@functools.lru_cache(None)
def random_cases(n=RANDOM_BLOCK_LISTS):
    return tuple(P.deflate_random(n, 29))


def hold_to_pillow(cases, decode, exact):
    """cases: (name, file, Pillow's pixels or None, ...); decode(file) -> (status, pixels).  A file that is taken is one Pillow
    takes, with equal pixels; a file Pillow refuses has status 2.  exact: Pillow takes every file and so must the decoder;
    otherwise the names in STRICTER_THAN_PILLOW -- and no others -- are refused although Pillow takes them."""
    failures, stricter = [], []
    for case in cases:
        name, data, ref = case[0], case[1], case[2]
        st, out = decode(data)
        if ref is None:
            if st != 2:
                failures.append(f"{name}: Pillow refuses the file, status {st}")
        elif st == 0:
            if out.shape != ref.shape or not np.array_equal(out, ref):
                failures.append(f"{name}: pixels differ from Pillow's")
        elif exact or st != 2:
            failures.append(f"{name}: Pillow takes the file, status {st}")
        else:
            stricter.append(name)
    if not exact:
        failures += [f"{n}: refused although Pillow takes it, and not listed" for n in stricter if n not in STRICTER_THAN_PILLOW]
        failures += [f"{n}: listed as refused, but it is not" for n in STRICTER_THAN_PILLOW if n not in stricter]
    return failures


def test_hand_written_deflate_streams_decode_as_pillow_does():
    """Every stream of deflate_valid -- codes of 15 bits, codes of 1 / 2 / 286 and 1 / 2 / 30 symbols, empty and tiny blocks,
    every repeat count of a header, every length, both ends of every distance code, runs, overlaps, dependent copies, stored
    blocks behind every bit offset, every zlib window size -- has status 0 and Pillow's pixels."""
    L = _lib()
    cases = valid_cases()
    failures = hold_to_pillow(cases, lambda d: _decode(L, d), exact=True)
    assert not failures, failures[:10]
    assert len(cases) >= 240


def test_the_valid_set_holds_every_feature_it_is_there_for():
    """The census of what the writer wrote (counted by the writer) against the list of features the set exists for."""
    census = sum((c[3] for c in valid_cases()), P.D.Counter())
    missing = [f for f in P.deflate_valid_features() if not census[f]]
    assert not missing, missing
    assert len(P.deflate_valid_features()) > 1000


def test_invalid_deflate_streams_are_refused_where_pillow_refuses():
    """One stream per rule of RFC 1950 / 1951: the decoder's status is 0 only if Pillow opens the file, and then the pixels are
    equal; a file Pillow refuses has status 2.  Among them the incomplete codes zlib refuses: a single code of 2..15 bits,
    two or more codes, in each of the three alphabets."""
    L = _lib()
    cases = invalid_cases()
    failures = hold_to_pillow(cases, lambda d: _decode(L, d), exact=False)
    assert not failures, "\n".join(failures)
    refused_by_pillow = sum(1 for c in cases if c[2] is None)
    assert len(cases) >= 360 and refused_by_pillow >= 280
    # zlib's own verdict goes with Pillow's wherever the image is not complete before the fault
    assert all(not c[3] for c in cases if c[2] is None and not c[0].startswith("output_one_byte_short"))


def test_random_block_lists_decode_as_pillow_does():
    L = _lib()
    cases = random_cases()
    failures = hold_to_pillow(cases, lambda d: _decode(L, d), exact=True)
    assert not failures, failures[:10]
    assert len(cases) == RANDOM_BLOCK_LISTS


def test_rewritten_block_headers_are_taken_only_where_pillow_takes_them():
    """50 dynamic-block streams, 10 000 rewrites of single header fields, checksums set right so that only the deflate layer
    can object: what the decoder takes Pillow takes, with equal pixels; what Pillow refuses has status 2.  The decoder may
    refuse what Pillow takes only where zlib itself does not inflate the whole stream to exactly the image's bytes: Pillow
    stops reading at the last row, the decoder reads the stream to its end (the asymmetry of STRICTER_THAN_PILLOW).
    On the tree this test came with: 10 000 rewrites, Pillow takes 774, of which zlib inflates 766 whole, the decoder takes
    those 766."""
    L = _lib()
    total = pillow_ok = whole_ok = taken = 0
    failures = []
    for name, data, ref, whole in P.deflate_header_fuzz(50, 200, 41):
        st, out = _decode(L, data)
        total += 1
        pillow_ok += ref is not None
        whole_ok += ref is not None and whole
        taken += st == 0
        if st == 0 and (ref is None or out.shape != ref.shape or not np.array_equal(out, ref)):
            failures.append(f"{name}: taken, {'Pillow refuses it' if ref is None else 'pixels differ'}")
        elif st != 0 and (st != 2 or (ref is not None and whole)):
            failures.append(f"{name}: status {st}, Pillow {'refuses' if ref is None else 'takes'} it")
    print(f"header fuzz: {total} rewrites, Pillow takes {pillow_ok} ({whole_ok} of them whole streams), the decoder takes {taken}")
    assert not failures, failures[:10]
    assert total >= 10000 and pillow_ok >= 100 and taken == whole_ok


def test_sanitised_build(tmp_path_factory):
    """The host build under AddressSanitizer and UBSan, as a program of its own (the sanitiser's runtime linked in): the valid,
    the invalid and the random set -- statuses and pixels as the plain build's, and no report."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    work = tmp_path_factory.mktemp("png_san")
    exe = str(work / "png_san")
    base = [cxx, "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            os.path.join(root, "tests", "_png_san_main.cpp"), "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    L = _lib()
    cases = list(valid_cases()) + list(invalid_cases()) + list(random_cases())
    paths = []
    for k, c in enumerate(cases):
        paths.append(str(work / f"{k}.png"))
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
        assert line == f"{st} {zlib.adler32(out.tobytes()) if st == 0 else 1}", c[0]
