"""WebP test cases for the decoder of lossy files with an alpha plane (kobato-eyes_amd/csrc/ke_webpa_*.h, ke_webpa.hip), in five
families: (1) RGBA files Pillow writes, (2) files a libwebp encoder loaded through ctypes writes with the alpha settings
Pillow's options cannot reach, (3) hand-muxed files -- a "VP8 " payload of a Pillow RGB save wrapped in VP8X + an ALPH chunk
built here: raw and VP8L-coded planes with each of the four filters, the pre-processing bit, container variants --, (4) the
refusals with their expected status, (5) the committed copies under tests/golden/webpa/ with the sha256 of Pillow's pixels.
Pillow is the reference throughout."""
from __future__ import annotations

import ctypes as C
import glob
import hashlib
import io
import json
import os

import numpy as np
from PIL import Image

import _vp8l_write as V
import _webp_cases as W
import _webpl_cases as L
from _webp_cases import CORRUPT, OK, UNSUPPORTED, chunks, content, exif_blob, frame_size, load_libwebp, riff, vp8_of  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "webpa")
ALPHA_KINDS = ("ramp", "disc", "noise", "smooth", "blocks")
CENSUS: dict = {}


def pillow_pixels(data: bytes):
    """Pillow's pixels as it opens the file (HxWx4 for RGBA, HxWx3 for RGB), or None where Pillow does not decode it"""
    try:
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert im.mode in ("RGB", "RGBA"), im.mode
            return np.asarray(im)
    except AssertionError:
        raise
    except Exception:
        return None


def plane(rng, w: int, h: int, kind: str) -> np.ndarray:
    """ramp / disc / noise / smooth / blocks (fully transparent and fully opaque ones) / opaque alpha values (h x w)"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "ramp":
        return (xx * 255 // max(w - 1, 1)).astype(np.uint8)
    if kind == "disc":
        return np.where((xx - w / 2) ** 2 + (yy - h / 2) ** 2 < (max(min(w, h), 3) / 3) ** 2, 255, 0).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "smooth":
        return ((np.sin(xx / 9.0) + np.cos(yy / 7.0) + 2) * 63).astype(np.uint8)
    a = np.full((h, w), 255, np.uint8)
    if kind == "blocks":
        a[: max(h // 2, 1), : max(w // 2, 1)] = 0
        a[h // 2:, w // 2:] = 128 if min(w, h) > 8 else 0
    return a


def pillow_file(rgb: np.ndarray, alpha: np.ndarray, quality: int = 80, method: int = 4, alpha_quality: int = 100, exact: bool = False) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.dstack([rgb, alpha]), "RGBA").save(buf, "WEBP", quality=quality, method=method, alpha_quality=alpha_quality, exact=exact)
    return buf.getvalue()


def alph_of(data: bytes):
    return next((p for t, p in chunks(data) if t == b"ALPH"), None)


def header_byte(data: bytes):
    a = alph_of(data)
    return a[0] if a else None


SIZES = [(1, 1), (1, 17), (17, 1), (2, 2), (3, 5), (15, 16), (16, 16), (17, 17), (31, 33), (64, 48), (99, 101), (255, 7), (200, 131), (512, 512),
         (513, 300)]


def pillow_cases(seed: int = 0, n: int = 90) -> list:
    """Family 1, [(name, bytes)]: alpha content ramp / disc / noise / smooth / blocks x method 0 / 4 / 6 x alpha_quality 100 and
    below x exact on and off, 1x1 through odd sizes to 512 x 512 and beyond.  (A fully opaque plane makes Pillow write a file
    without alpha: see opaque_cases.)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = SIZES[i] if i < len(SIZES) else (int(rng.integers(1, 260)), int(rng.integers(1, 260)))
        kind = ALPHA_KINDS[i % len(ALPHA_KINDS)]
        m, aq, ex = (0, 4, 6)[(i // 5) % 3], (100, 100, 60, 10)[(i // 15 + i) % 4], bool((i // 2) % 2)
        q = int(rng.integers(5, 100))
        data = pillow_file(content(rng, w, h, W.KINDS[(i // 3) % 5]), plane(rng, w, h, kind), q, m, aq, ex)
        out.append((f"pil_{i}_{kind}_{w}x{h}_q{q}_m{m}_aq{aq}_ex{int(ex)}", data))
    return out


def opaque_cases(seed: int = 5) -> list:
    """RGBA images whose plane is 255 throughout: Pillow writes them without alpha, so they are the lossy decoder's files."""
    rng = np.random.default_rng(seed)
    return [(f"opaque_{w}x{h}", pillow_file(content(rng, w, h, "smooth"), plane(rng, w, h, "opaque"), 70, 4)) for w, h in ((40, 30), (9, 70))]


# ---- libwebp's own encoder through ctypes ---------------------------------------------------------------------------------
def libwebp_file(lib, rgba: np.ndarray, *, quality=75, method=4, alpha_compression=1, alpha_filtering=1, alpha_quality=100, exact=0) -> bytes:
    cfg = W._Config()
    assert lib.WebPConfigInitInternal(C.byref(cfg), 0, C.c_float(quality), W._ENC_ABI)
    cfg.method, cfg.alpha_compression, cfg.alpha_filtering, cfg.alpha_quality, cfg.exact = method, alpha_compression, alpha_filtering, alpha_quality, exact
    assert lib.WebPValidateConfig(C.byref(cfg))
    pic = W._Picture()
    assert lib.WebPPictureInitInternal(C.byref(pic), W._ENC_ABI)
    h, w = rgba.shape[:2]
    pic.width, pic.height = w, h
    px = np.ascontiguousarray(rgba)
    assert lib.WebPPictureImportRGBA(C.byref(pic), px.ctypes.data_as(C.c_void_p), w * 4)
    mw = W._MemWriter()
    lib.WebPMemoryWriterInit(C.byref(mw))
    pic.writer = C.cast(lib.WebPMemoryWrite, C.c_void_p).value
    pic.custom_ptr = C.addressof(mw)
    try:
        assert lib.WebPEncode(C.byref(cfg), C.byref(pic)), f"WebPEncode failed ({pic.error_code})"
        return C.string_at(mw.mem, mw.size)
    finally:
        lib.WebPPictureFree(C.byref(pic))
        lib.WebPMemoryWriterClear(C.byref(mw))


def libwebp_cases(lib, seed: int = 3, n: int = 48) -> list:
    """Family 2, [(name, bytes)]: alpha_compression 0 / 1, alpha_filtering 0 (none) / 1 (fast) / 2 (best), alpha_quality 0..100"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = int(rng.integers(1, 140)), int(rng.integers(1, 140))
        kind = ALPHA_KINDS[i % len(ALPHA_KINDS)]
        rgba = np.dstack([content(rng, w, h, W.KINDS[(i // 2) % 5]), plane(rng, w, h, kind)])
        opts = dict(quality=int(rng.integers(0, 101)), method=i % 7, alpha_compression=int(i % 4 != 3), alpha_filtering=(i // 4) % 3,
                    alpha_quality=(100, 80, 30, 100, 0)[i % 5], exact=(i // 3) % 2)
        tag = "_".join(f"{k.split('_')[-1][:4]}{int(v)}" for k, v in opts.items())
        out.append((f"enc_{i}_{kind}_{w}x{h}_{tag}", libwebp_file(lib, rgba, **opts)))
    return out


# ---- hand-muxed files -----------------------------------------------------------------------------------------------------
def forward_filter(a: np.ndarray, filt: int) -> np.ndarray:
    """What an encoder stores for the plane ``a``: value - predictor (mod 256), the predictor as the container specification
    gives it (0 at the corner, left along row 0, above along column 0)."""
    if filt == 0:
        return a.copy()
    v = a.astype(np.int32)
    h, w = v.shape
    pred = np.zeros_like(v)
    pred[0, 1:] = v[0, :-1]
    pred[1:, 0] = v[:-1, 0]
    if h > 1 and w > 1:
        left, above, corner = v[1:, :-1], v[:-1, 1:], v[:-1, :-1]
        pred[1:, 1:] = left if filt == 1 else above if filt == 2 else np.clip(left + above - corner, 0, 255)
    return ((v - pred) & 255).astype(np.uint8)


def inverse_filter(stored: np.ndarray, filt: int) -> np.ndarray:
    """The plane a decoder makes of the stored bytes, pixel by pixel in raster order (the tests' own restatement)"""
    if filt == 0:
        return stored.copy()
    h, w = stored.shape
    out = np.zeros((h, w), np.int32)
    s = stored.astype(np.int32)
    for y in range(h):
        for x in range(w):
            if y == 0:
                p = out[0, x - 1] if x else 0
            elif x == 0:
                p = out[y - 1, 0]
            else:
                l, t, tl = out[y, x - 1], out[y - 1, x], out[y - 1, x - 1]
                p = l if filt == 1 else t if filt == 2 else min(max(l + t - tl, 0), 255)
            out[y, x] = (s[y, x] + p) & 255
    return out.astype(np.uint8)


def mux(vp8: bytes, alph, flags: int = 0x10, canvas=None, before=(), between=(), after=()) -> bytes:
    """RIFF / WEBP / VP8X / [before] / ALPH (``alph``: the chunk's bytes, None: no chunk) / [between] / "VP8 " / [after]"""
    w, h = canvas or frame_size(vp8)
    hdr = bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    return riff([(b"VP8X", hdr), *before, *([(b"ALPH", alph)] if alph is not None else []), *between, (b"VP8 ", vp8), *after])


def frame(rng, w: int, h: int, kind: str = "smooth", quality: int = 75) -> bytes:
    return vp8_of(W.pillow_file(content(rng, w, h, kind), quality, 4))


def raw_alph(a: np.ndarray, filt: int, pre: int = 0) -> bytes:
    return bytes([(pre << 4) | (filt << 2)]) + forward_filter(a, filt).tobytes()


def lossless_alph(vp8l_file: bytes, filt: int, pre: int = 0) -> bytes:
    """An ALPH chunk whose plane is coded as the VP8L stream of ``vp8l_file`` without its five header bytes"""
    return bytes([(pre << 4) | (filt << 2) | 1]) + L.vp8l_of(vp8l_file)[5:]


def raw_cases(seed: int = 21) -> list:
    """[(name, bytes, expected plane)]: raw planes with each of the four filters, the pre-processing bit, trailing bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (w, h) in enumerate([(1, 1), (1, 9), (9, 1), (2, 2), (33, 17), (64, 64), (70, 129), (257, 3)]):
        for filt in range(4):
            a = plane(rng, w, h, ALPHA_KINDS[(i + filt) % 5])
            out.append((f"raw_{w}x{h}_f{filt}", mux(frame(rng, w, h), raw_alph(a, filt, pre=int(i % 3 == 1))), a))
    a = plane(rng, 40, 30, "noise")
    out.append(("raw_trailing", mux(frame(rng, 40, 30), raw_alph(a, 3) + b"trailing bytes"), a))
    return out


def lossless_cases(seed: int = 22) -> list:
    """[(name, bytes, expected plane)]: VP8L-coded planes, each of the four filters over the test writer's forced-feature
    streams (colour indexing with packing, predictor, cross-colour, subtract-green, colour cache, LZ77, entropy image) and over
    Pillow's own lossless saves of the filtered plane"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (name, data, expected) in enumerate(V.written_cases()):
        h, w = expected.shape[:2]
        for filt in ((k % 4,) if k % 5 else range(4)):
            stored = expected[..., 1]                              # the green channel is what the stream stores
            out.append((f"vp8l_{name}_f{filt}", mux(frame(rng, w, h, "flat" if k % 2 else "smooth"), lossless_alph(data, filt, pre=int(k % 7 == 3))),
                        inverse_filter(stored, filt)))
    for i, (w, h) in enumerate([(1, 1), (5, 3), (47, 31), (128, 128), (301, 77)]):
        for filt in range(4):
            a = plane(rng, w, h, ALPHA_KINDS[(i + filt) % 5])
            g = forward_filter(a, filt)
            src = L.pillow_file(Image.fromarray(np.dstack([g // 2, g, 255 - g])), 60, (i + filt) % 7)
            out.append((f"vp8l_pillow_{w}x{h}_f{filt}", mux(frame(rng, w, h), lossless_alph(src, filt)), a))
    return out


def container_cases(seed: int = 23) -> list:
    """[(name, bytes, expected plane)]: the flag alone (alpha 255), ICCP / EXIF / XMP chunks around the image"""
    rng = np.random.default_rng(seed)
    out = []
    icc, xmp = b"\0" * 131, b"<x:xmpmeta xmlns:x='adobe:ns:meta/'/>"
    for i, (w, h) in enumerate([(1, 1), (40, 30), (100, 37)]):
        out.append((f"flag_alone_{w}x{h}", mux(frame(rng, w, h), None), np.full((h, w), 255, np.uint8)))
    a = plane(rng, 52, 41, "smooth")
    v = frame(rng, 52, 41)
    out.append(("iccp", mux(v, raw_alph(a, 1), 0x30, before=[(b"ICCP", icc)]), a))
    out.append(("exif", mux(v, raw_alph(a, 2), 0x18, after=[(b"EXIF", exif_blob())]), a))
    out.append(("iccp_exif_xmp", mux(v, raw_alph(a, 3), 0x3C, before=[(b"ICCP", icc)], after=[(b"EXIF", exif_blob(3)), (b"XMP ", xmp)]), a))
    out.append(("xmp_flag_alone", mux(v, None, 0x14, after=[(b"XMP ", xmp)]), np.full((41, 52), 255, np.uint8)))
    out.append(("opaque_raw", mux(v, raw_alph(np.full((41, 52), 255, np.uint8), 0)), np.full((41, 52), 255, np.uint8)))
    return out


def muxed_cases() -> list:
    """Family 3, [(name, bytes, expected plane)]"""
    return raw_cases() + lossless_cases() + container_cases()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def refused_cases(seed: int = 2) -> list:
    """Family 4, [(name, bytes, expected status)] of files the decoder leaves to Pillow"""
    rng = np.random.default_rng(seed)
    w, h = 40, 30
    rgb = content(rng, w, h, "smooth")
    v = vp8_of(W.pillow_file(rgb, 80, 4))
    a = plane(rng, w, h, "smooth")
    good = raw_alph(a, 1)
    out = [("plain_lossy", W.pillow_file(rgb, 80, 4), UNSUPPORTED), ("plain_lossy_vp8x", W.vp8x(v), UNSUPPORTED)]
    out += [(n, d, UNSUPPORTED) for n, d in opaque_cases()]
    out.append(("lossless", L.pillow_file(Image.fromarray(np.dstack([rgb, a]), "RGBA")), UNSUPPORTED))
    body = L.vp8l_of(L.pillow_file(Image.fromarray(rgb)))
    hdr = bytes([0x10, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    out.append(("lossless_with_alph", riff([(b"VP8X", hdr), (b"ALPH", good), (b"VP8L", body)]), UNSUPPORTED))
    frames = [Image.fromarray(np.dstack([content(rng, 32, 32, k), plane(rng, 32, 32, "disc")]), "RGBA") for k in ("smooth", "noisy")]
    buf = io.BytesIO()
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], quality=70, duration=100)
    out.append(("animated", buf.getvalue(), UNSUPPORTED))
    out.append(("animation_flag", mux(v, good, 0x12), UNSUPPORTED))
    out.append(("alph_without_flag", mux(v, good, 0x00), UNSUPPORTED))
    out.append(("canvas_mismatch", mux(v, good, canvas=(w + 1, h)), UNSUPPORTED))
    out.append(("unknown_chunk", mux(v, good, after=[(b"ZZZZ", b"1234")]), UNSUPPORTED))
    out.append(("chunk_between_plane_and_frame", mux(v, good, 0x18, between=[(b"EXIF", exif_blob())]), UNSUPPORTED))
    inter = bytearray(v)
    inter[0] |= 1
    out.append(("inter_frame", mux(bytes(inter), good), UNSUPPORTED))
    giant = bytearray(v)                                        # 4097 x 4097: over the lossy decoder's cap
    giant[6:10] = (4097).to_bytes(2, "little") * 2
    out.append(("over_pixel_cap", mux(bytes(giant), None), UNSUPPORTED))
    # what Pillow fails on
    out.append(("two_alph", mux(v, good, between=[(b"ALPH", good)]), CORRUPT))
    out.append(("alph_behind_frame", mux(v, None, after=[(b"ALPH", good)]), CORRUPT))
    out.append(("raw_short", mux(v, good[:-1]), CORRUPT))
    out.append(("raw_half", mux(v, good[: len(good) // 2]), CORRUPT))
    out.append(("method_2", mux(v, bytes([good[0] | 2]) + good[1:]), CORRUPT))
    out.append(("method_3", mux(v, bytes([good[0] | 3]) + good[1:]), CORRUPT))
    out.append(("pre_2", mux(v, bytes([good[0] | 0x20]) + good[1:]), CORRUPT))
    out.append(("pre_3", mux(v, bytes([good[0] | 0x30]) + good[1:]), CORRUPT))
    out.append(("reserved_bit", mux(v, bytes([good[0] | 0x40]) + good[1:]), CORRUPT))
    out.append(("reserved_bit_upper", mux(v, bytes([good[0] | 0x80]) + good[1:]), CORRUPT))
    out.append(("empty_chunk", mux(v, b""), CORRUPT))
    out.append(("one_byte_chunk", mux(v, b"\0"), CORRUPT))
    src = L.pillow_file(Image.fromarray(np.dstack([forward_filter(plane(rng, w, h, "noise"), 0)] * 3)), 60, 4)
    whole = lossless_alph(src, 0)
    out.append(("vp8l_plane_cut_in_half", mux(v, whole[: len(whole) // 2]), CORRUPT))
    lossy = mux(v, good)
    out.append(("truncated_half", lossy[: len(lossy) // 2], CORRUPT))
    big = bytearray(lossy)
    big[4:8] = (len(lossy) + 100).to_bytes(4, "little")
    out.append(("riff_too_long", bytes(big), CORRUPT))
    return out


# ---- the committed files --------------------------------------------------------------------------------------------------
def golden_cases() -> list:
    """Family 5, [(name, bytes, sha256 of Pillow's RGBA pixels when the file was committed)]"""
    index = os.path.join(GOLDEN, "index.json")
    if not os.path.exists(index):
        return []
    with open(index) as f:
        want = json.load(f)
    return [(name, open(os.path.join(GOLDEN, name), "rb").read(), want[name]) for name in sorted(want)]


def all_taken(lib=None) -> list:
    """[(family, name, bytes)] of every file of families 1-3 and 5 (2 where the encoder is at hand)"""
    out = [(1, n, d) for n, d in pillow_cases()]
    if lib is not None:
        out += [(2, n, d) for n, d in libwebp_cases(lib)]
    out += [(3, n, d) for n, d, _ in muxed_cases()]
    out += [(5, n, d) for n, d, _ in golden_cases()]
    return out


# ---- damage ---------------------------------------------------------------------------------------------------------------
def fuzz_bases(seed: int = 7) -> list:
    """16 Pillow-written files of 33x17 .. 120x90 and 8 hand-muxed ones (raw and VP8L planes, every filter) for the damage fuzz"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(16):
        w, h = int(rng.integers(33, 121)), int(rng.integers(17, 91))
        out.append(pillow_file(content(rng, w, h, W.KINDS[i % 5]), plane(rng, w, h, ALPHA_KINDS[i % 5]), int(rng.integers(20, 100)), (0, 4, 6)[i % 3],
                               (100, 100, 50)[i % 3]))
    for filt in range(4):
        a = plane(rng, 48, 36, ALPHA_KINDS[filt])
        g = forward_filter(a, filt)
        out.append(mux(frame(rng, 48, 36), raw_alph(a, filt)))
        out.append(mux(frame(rng, 48, 36), lossless_alph(L.pillow_file(Image.fromarray(np.dstack([g, g, g])), 50, 3), filt)))
    return out


def damaged(data: bytes, rng, count: int) -> list:
    """Mutations of one file between offset 12 and the end of its ALPH chunk (the end of the file where it has none): one to
    three bits flipped, a byte overwritten, a cut, a byte run deleted or inserted"""
    at = data.find(b"ALPH")
    end = at + 8 + int.from_bytes(data[at + 4:at + 8], "little") if at >= 0 else len(data)
    end = min(max(end, 13), len(data))
    out = []
    for _ in range(count):
        b = bytearray(data)
        op = int(rng.integers(0, 8))
        if op <= 2:
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(12, end))] ^= 1 << int(rng.integers(0, 8))
        elif op <= 4:
            b[int(rng.integers(12, end))] = int(rng.integers(0, 256))
        elif op == 5:
            b = b[: int(rng.integers(12, end))]
        elif op == 6:
            k = int(rng.integers(12, end))
            b[k:k] = rng.integers(0, 256, int(rng.integers(1, 5)), dtype=np.uint8).tobytes()
        else:
            k = int(rng.integers(12, end - 1))
            del b[k:k + int(rng.integers(1, 5))]
        out.append(bytes(b))
    return out


def write_golden(lib) -> None:
    """(maintenance) regenerate tests/golden/webpa/: small files of families 1-3 and the sha256 of Pillow's pixels"""
    os.makedirs(GOLDEN, exist_ok=True)
    picks = [(f"pil_{k:02d}.webp", d) for k, (_, d) in enumerate(pillow_cases(seed=40, n=14)) if len(d) < 20000]
    picks += [(f"enc_{k:02d}.webp", d) for k, (_, d) in enumerate(libwebp_cases(lib, seed=41, n=14))]
    third = muxed_cases()
    picks += [(f"mux_{k:02d}.webp", third[j][1]) for k, j in enumerate(range(0, len(third), max(1, len(third) // 14)))][:14]
    want = {}
    for name, data in picks:
        px = pillow_pixels(data)
        assert px is not None and px.shape[2] == 4, name
        with open(os.path.join(GOLDEN, name), "wb") as f:
            f.write(data)
        want[name] = hashlib.sha256(px.tobytes()).hexdigest()
    with open(os.path.join(GOLDEN, "index.json"), "w") as f:
        json.dump(want, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    lib = load_libwebp()
    if lib is None:
        raise SystemExit("no libwebp encoder here")
    write_golden(lib)
