"""The product's JPEG arithmetic (csrc/ke_jpeg_core.h + ke_jpeg_parse.h, the headers the HIP kernels compile) built for the
host (oracle/libkeyes_jpeg_cpu.so) against the installed Pillow: pixel-exact on every file the decoder takes, and the right
refusal for the rest.  The GPU kernels are then held against Pillow directly (tests/test_gpu_jpeg.py)."""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np
from PIL import Image

import _jpeg_cases as J
from oracle import oracle as O


def _lib():
    path = os.path.join(os.path.dirname(O.__file__), "libkeyes_jpeg_cpu.so")
    if not os.path.exists(path):
        O.build(force=True)                                 # make -B builds both libraries of oracle/
    L = C.CDLL(path)
    L.ko_jpeg_probe.argtypes = [C.c_void_p, C.c_uint64] + [C.POINTER(C.c_int32)] * 3
    L.ko_jpeg_decode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def _decode(L, data: bytes):
    buf = np.frombuffer(data + b"\0", np.uint8)          # never a zero-length array
    w, h, ch = C.c_int32(), C.c_int32(), C.c_int32()
    st = L.ko_jpeg_probe(buf.ctypes.data, len(data), C.byref(w), C.byref(h), C.byref(ch))
    if st:
        return st, None
    out = np.empty((h.value, w.value, 3) if ch.value == 3 else (h.value, w.value), np.uint8)
    return L.ko_jpeg_decode(buf.ctypes.data, len(data), out.ctypes.data), out


def test_decoder_arithmetic_matches_pillow():
    L = _lib()
    n = 0
    for name, data, ref in J.supported():
        st, out = _decode(L, data)
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name
        n += 1
    assert n > 150


def test_blocks_beyond_the_idct_bound_hand_the_file_back():
    """ke_idct_islow's bound: with the quantisation tables overwritten by larger and larger steps the decode is Pillow's until
    a block leaves 16 bits, and KE_JPEG_UNSUPPORTED from there (libjpeg's C form and Pillow's SIMD build differ beyond)."""
    L = _lib()
    good = [c for c in J.supported() if c[2].shape[0] >= 64 and "gray" not in c[0]][:6] + [c for c in J.supported() if "q100" in c[0] and c[2].shape[0] >= 64][:2]
    taken = {}
    for _, data, _ in good:
        for v in (255, 16, 4, 1):
            blob = J.with_quantisation_tables(data, v)
            st, out = _decode(L, blob)
            assert st in (0, 1)
            if st == 0:
                assert np.array_equal(out, np.asarray(Image.open(io.BytesIO(blob))))
            taken[v] = taken.get(v, 0) + (st == 0)
    assert taken[255] == 0 and taken[1] == len(good) and 0 < taken[16] < len(good)


def test_damaged_files_the_decoder_takes_are_decoded_as_pillow_does():
    """tests/fuzz_jpeg_damage.py, a bounded sample: one header byte changed / the entropy data flipped, overwritten, cut, with
    bytes deleted or inserted.  A file the decoder still takes has Pillow's pixels (reserved markers, bad segment lengths, bad
    sampling factors, unusable Huffman tables, renumbered or missing restart markers, data that runs dry are all refused: libjpeg
    stops on the former and patches the latter up by heuristics of its own)."""
    import fuzz_jpeg_damage as F

    cases, taken, wrong = F.check(F.cpu_decoder(), 12, 7, files=30)
    assert not wrong, wrong[:5]
    assert cases == 1080 and taken > 150


def test_files_outside_the_decoder_are_refused():
    L = _lib()
    for name, data, expected in J.refused():
        st, _ = _decode(L, data)
        assert st == expected, name


def test_quad_upsampler_equals_the_per_sample_one():
    """ke_upsample4 (the colour kernel's) == ke_upsample_at (the one held against Pillow above) for every component width 1..21,
    height 1..9 and sampling 1x1 / 2x1 / 2x2."""
    assert _lib().ko_jpeg_upsample_selftest() == 0


def test_random_files_decode_as_pillow_does():
    """Property: whatever Pillow (libjpeg-turbo) writes as a Huffman JPEG -- any size up to 90 x 70, grayscale or colour at
    4:4:4 / 4:2:2 / 4:2:0, any quality, sequential or progressive, optimised tables or not, restart intervals -- the decoder
    arithmetic yields Pillow's pixels."""
    import io

    from hypothesis import given, settings
    from hypothesis import strategies as st
    from PIL import Image

    L = _lib()

    @settings(max_examples=120, deadline=None, derandomize=True)
    @given(st.integers(1, 90), st.integers(1, 70), st.booleans(), st.integers(0, 2), st.integers(1, 100), st.booleans(), st.booleans(),
           st.integers(0, 9), st.integers(0, 2), st.integers(0, 2 ** 32 - 1))
    def check(w, h, gray, sub, quality, progressive, optimize, restart, texture, seed):
        rng = np.random.default_rng(seed)
        if texture == 0:
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif texture == 1:
            a = np.repeat(np.repeat(rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8), 8, 0), 8, 1)[:h, :w]
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            a = np.stack([xx * 3 % 256, yy * 5 % 256, (xx + yy) % 256], -1).astype(np.uint8)
        kw = {"quality": quality, "progressive": progressive, "optimize": optimize}
        if not gray:
            kw["subsampling"] = sub
        if restart:
            kw["restart_marker_blocks"] = restart
        b = io.BytesIO()
        try:
            Image.fromarray(a[:, :, 0] if gray else a).save(b, "JPEG", **kw)
        except TypeError:                                   # a Pillow without the restart options
            kw.pop("restart_marker_blocks")
            Image.fromarray(a[:, :, 0] if gray else a).save(b, "JPEG", **kw)
        data = b.getvalue()
        ref = np.asarray(Image.open(io.BytesIO(data)))
        status, out = _decode(L, data)
        assert status == 0 and out.shape == ref.shape and np.array_equal(out, ref)

    check()


def test_progressive_files_with_any_scan_script_decode_as_pillow_does():
    """Pillow's writer only knows libjpeg's default progression; other encoders (mozjpeg: what most image hosts serve) cut and
    order their scans differently.  120 files with random legal scripts (tests/_jpeg_prog_encoder.py: DC scans for one, some or
    all components, AC bands cut anywhere, successive approximation from any bit, scans shuffled as far as T.81 allows)."""
    L = _lib()
    n = 0
    for name, data, ref in J.scripted(120, 5):
        st, out = _decode(L, data)
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name
        n += 1
    assert n == 120


# ---- hand-written entropy streams (tests/_jpeg_write.py, tests/_jpeg_stream_cases.py) ----------------------------------------------
def test_hand_written_streams_cover_what_they_are_for():
    """The coverage assertions of every family, from the writer's facts: code lengths 1..16 for DC and AC symbols, the 9/10-bit
    edge, stuffed pairs at every window offset, the EOI at every lane and step edge of the end search, EOB0..EOB14, ..."""
    import _jpeg_stream_cases as S

    counts = S.coverage()
    assert sum(counts.values()) == len(S.valid()) and min(counts.values()) >= 10, counts


def test_valid_hand_written_streams_decode_as_pillow_does():
    """Every V case is taken, with Pillow's shape and pixels: nothing is left out."""
    import _jpeg_stream_cases as S

    L = _lib()
    refs = S.references()
    for name, data, _ in S.valid():
        ref = refs[name]
        assert ref is not None, name
        st, out = _decode(L, data)
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name


def test_tolerated_streams_get_their_pinned_status_or_pillows_pixels():
    """What libjpeg patches up without an error: Pillow yields pixels, the decoder gives the pinned status -- and where that is
    0, Pillow's pixels."""
    import _jpeg_stream_cases as S

    L = _lib()
    refs = S.references()
    for name, data, expected, why in S.tolerated():
        assert refs[name] is not None, name
        st, out = _decode(L, data)
        assert st == expected, (name, st, why)
        if st == 0:
            assert out.shape == refs[name].shape and np.array_equal(out, refs[name]), name
    assert len(S.tolerated()) == 13


def test_unusable_huffman_tables_are_refused_where_pillow_raises():
    import _jpeg_stream_cases as S

    L = _lib()
    for name, data in S.refused():
        assert S.pillow(data) is None, name
        assert _decode(L, data)[0] == 2, name
    assert len(S.refused()) == 5


def test_progressive_encoder_still_writes_the_same_files():
    """tests/_jpeg_prog_encoder.py goes through tests/_jpeg_write.py now: the files of J.scripted and E.random_file are the ones
    from before, byte for byte (the census pinned in fuzz_jpeg_damage and the scripted tests depend on them)."""
    import hashlib

    import _jpeg_prog_encoder as E

    h = hashlib.sha256()
    for _, data, _ in J.scripted(120, 5):
        h.update(data)
    assert h.hexdigest() == "4ea1c80e73af5a8154369c3052d092cc99c0c759f3072e3f695e75008594b143"
    h = hashlib.sha256()
    rng = np.random.default_rng(77)
    for k in range(40):
        h.update(E.random_file(rng, 10 + k, 7 + k, ("444", "422", "420", "440")[k % 4], k % 5 == 0)[0])
    assert h.hexdigest() == "2d981e17b932967bf1e2d3dd98420a225c24a29f94d4ddf5113898967a44bfda"


# ---- hand-written files for the IDCT bound, the planes' padding and the colour cube (tests/_jpeg_sample_cases.py) --------------------
def test_sample_cases_cover_what_they_are_for():
    """From the coefficients and from Pillow alone: 600+ blocks within 1 384 of the bound on the inside, 300+ files with one
    block within 1 116 on the outside, both signs, both shortcuts, every component and block position; padding that differs
    from the last real column / row in every padded file, chroma samples of 0 and 255 and steps of 100 in 100+ files each;
    all 65 536 pairs of the two ramp planes in every colour file."""
    import _jpeg_sample_cases as C

    fig = C.coverage()
    assert fig["taken_blocks"] >= 600 and fig["handed_back_blocks"] >= 300, fig
    assert max(fig["closest_inside"].values()) <= 8 and max(fig["closest_outside"].values()) <= 8, fig
    assert all(n == 65536 for name, n in fig["colour_pairs"].items() if name.endswith("noise")), fig


def test_extremes_predicts_the_host_builds_status_for_every_bound_case():
    """The plain-integer restatement of what ke_idct_islow tracks (C.extremes, which built the cases) and the host build agree
    on which side of the bound every file lies: 0 for a file whose blocks are all narrow, 1 for one with a block outside."""
    import _jpeg_sample_cases as C

    L = _lib()
    n = [0, 0]
    for name, data, facts in C.bound_cases():
        tq = [c[3] for c in facts.comps] if hasattr(facts, "comps") else [0, 1, 1]
        predicted = int(not all(C.narrow(plane[at], facts.q[tq[j]]) for j, plane in enumerate(facts.coefs) for at in np.ndindex(plane.shape[:2])))
        assert predicted == facts.status, name
        assert _decode(L, data)[0] == predicted, name
        n[predicted] += 1
    assert n[0] >= 300 and n[1] >= 350, n


def test_taken_padding_and_colour_cases_decode_as_pillow_does():
    """The host build takes every file inside the bound, every padding file and every colour file with Pillow's pixels, and
    hands back every file with a block outside (status 1)."""
    import _jpeg_sample_cases as C

    L = _lib()
    refs = C.references()
    for name, data, facts in C.bound_cases() + C.padding_cases() + C.colour_cases():
        st, out = _decode(L, data)
        ref = refs[name]
        assert ref is not None, name
        if getattr(facts, "status", 0):
            assert st == 1, name
            continue
        assert st == 0, name
        assert out.shape == ref.shape and np.array_equal(out, ref), name
