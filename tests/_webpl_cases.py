"""WebP test cases for the lossless decoder (kobato-eyes_amd/csrc/ke_webpl_*.h, ke_webpl.hip): files Pillow writes (RGB, L, P
with palettes of every packing width, RGBA with and without ``exact``), files a libwebp encoder loaded through ctypes writes
with settings Pillow's options cannot reach (near_lossless, use_delta_palette, image_hint), container variants, the refusals
with their expected status, and damage.  The committed copies under tests/golden/webpl/ -- written by the libwebp encoder --
let a run without that encoder hold the same ground."""
from __future__ import annotations

import ctypes as C
import glob
import io
import os
import struct

import numpy as np
from PIL import Image

import _webp_cases as W
from _webp_cases import CORRUPT, OK, UNSUPPORTED, KINDS, chunks, content, damaged, exif_blob, load_libwebp, riff  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "webpl")
MAX_PIXELS = 1 << 24


def pillow_pixels(data: bytes):
    """Pillow's pixels as it opens the file (HxWx3 for RGB, HxWx4 for RGBA), or None where Pillow does not decode it"""
    try:
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert im.mode in ("RGB", "RGBA"), im.mode
            return np.asarray(im)
    except AssertionError:
        raise
    except Exception:
        return None


def pillow_file(im: Image.Image, quality: int = 80, method: int = 4, **kw) -> bytes:
    buf = io.BytesIO()
    im.save(buf, "WEBP", lossless=True, quality=quality, method=method, **kw)
    return buf.getvalue()


def _rgba(rng, a: np.ndarray, opaque: bool = False) -> Image.Image:
    h, w = a.shape[:2]
    alpha = np.full((h, w, 1), 255, np.uint8) if opaque else rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    if not opaque:
        alpha[: h // 2, : w // 2] = 0                            # fully transparent pixels: kept only with exact=True
    return Image.fromarray(np.concatenate([a, alpha], -1), "RGBA")


SIZES = [(1, 1), (1, 17), (17, 1), (2, 2), (3, 5), (15, 16), (16, 16), (17, 17), (31, 33), (64, 48), (99, 101), (255, 7)]


def pillow_cases(seed: int = 0, n: int = 140) -> list:
    """[(name, bytes)]: content kinds x methods 0..6 x qualities x sizes 1x1 .. ~1000; RGB, L, P (2, 3-4, 5-16, 17-256 colours),
    RGBA with and without exact=True, opaque RGBA"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i < len(SIZES):
            w, h = SIZES[i]
        elif i % 29 == 0:
            w, h = int(rng.integers(600, 1000)), int(rng.integers(200, 500))
        else:
            w, h = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        kind = KINDS[i % len(KINDS)]
        q, m = int(rng.integers(0, 101)), i % 7
        a = content(rng, w, h, kind)
        form = ("rgb", "rgb", "L", "P", "rgba", "rgba_exact", "rgba_opaque", "rgb")[(i // 5) % 8]
        kw = {}
        if form == "L":
            im = Image.fromarray(a).convert("L")
        elif form == "P":
            colours = (2, 4, 3, 16, 9, 256, 40)[(i // 40 + i) % 7]
            im = Image.fromarray(a if kind != "flat" else content(rng, w, h, "noisy")).quantize(colours)
        elif form.startswith("rgba"):
            im = _rgba(rng, a, opaque=form == "rgba_opaque")
            kw["exact"] = form == "rgba_exact"
        else:
            im = Image.fromarray(a)
        out.append((f"pil_{i}_{kind}_{form}_{w}x{h}_q{q}_m{m}", pillow_file(im, q, m, **kw)))
    return out


def palette_cases(seed: int = 6) -> list:
    """P images with exactly 2, 3, 4, 5, 16, 17 and 256 colours in use: every packing width"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (2, 3, 4, 5, 16, 17, 256):
        w, h = int(rng.integers(20, 90)), int(rng.integers(20, 90))
        im = Image.fromarray(rng.integers(0, n, (h, w), dtype=np.uint8), "P")
        im.putpalette(rng.integers(0, 256, 768, dtype=np.uint8).tobytes())
        out.append((f"palette_{n}_{w}x{h}", pillow_file(im, 70, 4)))
    return out


# ---- libwebp's own encoder through ctypes ---------------------------------------------------------------------------------
def libwebp_file(lib, a: np.ndarray, *, quality=75, method=4, near_lossless=100, exact=0, delta_palette=0, hint=0) -> bytes:
    cfg = W._Config()
    assert lib.WebPConfigInitInternal(C.byref(cfg), 0, C.c_float(quality), W._ENC_ABI)
    cfg.lossless, cfg.method, cfg.near_lossless, cfg.exact, cfg.use_delta_palette, cfg.image_hint = 1, method, near_lossless, exact, delta_palette, hint
    assert lib.WebPValidateConfig(C.byref(cfg))
    pic = W._Picture()
    assert lib.WebPPictureInitInternal(C.byref(pic), W._ENC_ABI)
    h, w = a.shape[:2]
    pic.width, pic.height, pic.use_argb = w, h, 1
    px = np.ascontiguousarray(a)
    imp = lib.WebPPictureImportRGBA if a.shape[2] == 4 else lib.WebPPictureImportRGB
    assert imp(C.byref(pic), px.ctypes.data_as(C.c_void_p), w * a.shape[2])
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


def libwebp_cases(lib, seed: int = 3, n: int = 36) -> list:
    """[(name, bytes)]: near_lossless 0..100, exact, use_delta_palette, image_hint 0..3, with and without alpha"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        kind = KINDS[i % len(KINDS)]
        a = content(rng, w, h, kind)
        if i % 3 == 2:
            a = np.concatenate([a, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
        opts = dict(quality=int(rng.integers(0, 101)), method=i % 7, near_lossless=(100, 60, 40, 0)[i % 4], exact=(i // 2) % 2,
                    delta_palette=int(i % 9 == 4), hint=i % 4)
        tag = "_".join(f"{k[:4]}{int(v)}" for k, v in opts.items())
        out.append((f"enc_{i}_{kind}_{w}x{h}_{tag}", libwebp_file(lib, a, **opts)))
    return out


def golden_cases() -> list:
    """[(name, bytes)] of the committed files"""
    return [(os.path.basename(p), open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(GOLDEN, "*.webp")))]


# ---- container variants -------------------------------------------------------------------------------------------------
def vp8l_of(data: bytes) -> bytes:
    return next(p for t, p in chunks(data) if t == b"VP8L")


def image_size(vp8l: bytes) -> tuple:
    bits = struct.unpack("<I", vp8l[1:5])[0]
    return (bits & 0x3FFF) + 1, ((bits >> 14) & 0x3FFF) + 1


def vp8x(vp8l: bytes, flags: int = 0, canvas=None, before=(), after=()) -> bytes:
    w, h = canvas or image_size(vp8l)
    hdr = bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    return riff([(b"VP8X", hdr), *before, (b"VP8L", vp8l), *after])


def wrapped_cases(seed: int = 1) -> list:
    """Extended-format files the decoder takes: VP8X with ICCP / EXIF / XMP chunks around the image, the alpha flag set or not
    (Pillow's mode follows the VP8L header's alpha bit, whatever the VP8X flag says)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(12):
        w, h = int(rng.integers(8, 120)), int(rng.integers(8, 120))
        a = content(rng, w, h, KINDS[i % 5])
        im = _rgba(rng, a) if i % 3 == 0 else Image.fromarray(a)
        body = vp8l_of(pillow_file(im, int(rng.integers(10, 95)), 4))
        icc, xmp = b"\0" * (128 + i), b"<x:xmpmeta xmlns:x='adobe:ns:meta/'/>"
        al = 0x10 if (i % 3 == 0) != (i % 4 == 3) else 0           # mostly as the image says, sometimes the other way round
        variants = [vp8x(body, al), vp8x(body, al | 0x20, before=[(b"ICCP", icc)]), vp8x(body, al | 0x08, after=[(b"EXIF", exif_blob())]),
                    vp8x(body, al | 0x2C, before=[(b"ICCP", icc)], after=[(b"EXIF", exif_blob(3)), (b"XMP ", xmp)])]
        out.append((f"vp8x_{i}_alpha{al >> 4}", variants[i % 4]))
    return out


def refused_cases(seed: int = 2) -> list:
    """[(name, bytes, expected status)] of files the decoder leaves to Pillow."""
    rng = np.random.default_rng(seed)
    a = content(rng, 40, 30, "smooth")
    good = pillow_file(Image.fromarray(a))
    body = vp8l_of(good)
    out = [("lossy", W.pillow_file(a, 80, 4), UNSUPPORTED)]
    buf = io.BytesIO()
    _rgba(rng, a).save(buf, "WEBP", quality=80)
    out.append(("lossy_with_alph", buf.getvalue(), UNSUPPORTED))
    frames = [Image.fromarray(content(rng, 32, 32, k)) for k in ("smooth", "noisy")]
    buf = io.BytesIO()
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], lossless=True, duration=100)
    out.append(("animated", buf.getvalue(), UNSUPPORTED))
    version = bytearray(body)
    version[4] |= 0x20
    out.append(("version_1", riff([(b"VP8L", bytes(version))]), UNSUPPORTED))
    w, h = image_size(body)
    out.append(("canvas_mismatch", vp8x(body, canvas=(w + 1, h)), UNSUPPORTED))
    out.append(("unknown_chunk", vp8x(body, after=[(b"ZZZZ", b"1234")]), UNSUPPORTED))
    out.append(("animation_flag", vp8x(body, 0x02), UNSUPPORTED))
    out.append(("two_images", vp8x(body, after=[(b"VP8L", body)]), UNSUPPORTED))
    giant = bytearray(body)                                   # 4097 x 4097: over the pixel cap
    giant[1:5] = struct.pack("<I", 4096 | (4096 << 14))
    out.append(("over_pixel_cap", riff([(b"VP8L", bytes(giant))]), UNSUPPORTED))
    out.append(("truncated_half", good[: len(good) // 2], CORRUPT))
    out.append(("truncated_header", good[:20], CORRUPT))
    big = bytearray(good)
    big[4:8] = struct.pack("<I", len(good) + 100)
    out.append(("riff_too_long", bytes(big), CORRUPT))
    short = riff([(b"VP8L", body[: len(body) // 2 & ~1])])      # the container is whole, the stream ends early
    out.append(("stream_ends_early", short, CORRUPT))
    sig = bytearray(body)
    sig[0] = 0x2E
    out.append(("bad_signature", riff([(b"VP8L", bytes(sig))]), CORRUPT))
    return out


def taken_cases() -> list:
    """Every case the decoder takes that needs no encoder beyond Pillow's, plus the committed ones."""
    return pillow_cases() + palette_cases() + wrapped_cases() + golden_cases()


def fuzz_bases(seed: int = 7) -> list:
    """15 Pillow-written lossless files of 33x17 .. 120x90 for the damage fuzz"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(15):
        w, h = int(rng.integers(33, 121)), int(rng.integers(17, 91))
        a = content(rng, w, h, KINDS[i % 5])
        im = _rgba(rng, a) if i % 5 == 4 else Image.fromarray(a).quantize(12) if i % 5 == 2 else Image.fromarray(a)
        out.append(pillow_file(im, int(rng.integers(20, 100)), i % 7))
    return out


def write_golden(lib) -> None:
    """(maintenance) regenerate tests/golden/webpl/ from the libwebp encoder cases"""
    os.makedirs(GOLDEN, exist_ok=True)
    for name, data in libwebp_cases(lib):
        with open(os.path.join(GOLDEN, "_".join(name.split("_")[:2]) + ".webp"), "wb") as f:
            f.write(data)


if __name__ == "__main__":
    lib = load_libwebp()
    if lib is None:
        raise SystemExit("no libwebp encoder here")
    write_golden(lib)
