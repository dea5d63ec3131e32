"""WebP test cases for the lossy decoder (kobato-eyes_amd/csrc/ke_webp_*.h, ke_webp.hip): files Pillow writes, files a libwebp
encoder loaded through ctypes writes with settings Pillow's options cannot reach (simple filter, filter level 0, sharpness,
token partitions, segments), container variants, the refusals with their expected status, and damage.  The committed copies
under tests/golden/webp/ let a run without that encoder hold the same ground."""
from __future__ import annotations

import ctypes as C
import ctypes.util
import glob
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "webp")


def content(rng, w: int, h: int, kind: str) -> np.ndarray:
    """noisy / smooth / flat / drawing / gray pixels (h x w x 3)"""
    if kind == "noisy":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        a = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 127 // max(w + h - 2, 1)], -1)
        return a.astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3).astype(np.uint8), (h, w, 3)).copy()
    if kind == "drawing":
        a = np.full((h, w, 3), 255, np.uint8)
        a[(yy // 7) % 3 == 0] = rng.integers(0, 256, 3)
        a[(xx * 3 + yy * 5) % 23 < 2] = 0
        return a
    g = ((xx * 7 + yy * 13) % 256).astype(np.uint8)                 # gray
    return np.stack([g, g, g], -1)


KINDS = ("noisy", "smooth", "flat", "drawing", "gray")


def pillow_file(a: np.ndarray, quality: int, method: int, **kw) -> bytes:
    buf = io.BytesIO()
    im = Image.fromarray(a)
    if kw.pop("gray", False):
        im = im.convert("L")
    im.save(buf, "WEBP", quality=quality, method=method, **kw)
    return buf.getvalue()


def pillow_cases(seed: int = 0, n: int = 160) -> list:
    """[(name, bytes)] of Pillow-encoded lossy files: quality 0..100, method 0..6, 1x1 .. ~1000 sides, odd sizes."""
    rng = np.random.default_rng(seed)
    out = []
    sizes = [(1, 1), (1, 17), (17, 1), (2, 2), (3, 5), (15, 16), (16, 16), (17, 17), (31, 33), (64, 48), (99, 101), (255, 7)]
    for i in range(n):
        if i < len(sizes):
            w, h = sizes[i]
        elif i % 23 == 0:
            w, h = int(rng.integers(600, 1000)), int(rng.integers(200, 500))
        else:
            w, h = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        kind = KINDS[i % len(KINDS)]
        q, m = int(rng.integers(0, 101)), int(rng.integers(0, 7))
        out.append((f"pil_{i}_{kind}_{w}x{h}_q{q}_m{m}", pillow_file(content(rng, w, h, kind), q, m, gray=kind == "gray" and i % 2 == 0)))
    return out


# ---- container surgery -------------------------------------------------------------------------------------------------
def chunks(data: bytes) -> list:
    """[(fourcc, payload)] of a RIFF/WEBP file"""
    out, pos = [], 12
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        out.append((tag, data[pos + 8:pos + 8 + size]))
        pos += 8 + size + (size & 1)
    return out


def riff(parts: list) -> bytes:
    body = b"".join(tag + struct.pack("<I", len(p)) + p + (b"\0" if len(p) & 1 else b"") for tag, p in parts)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


def vp8_of(data: bytes) -> bytes:
    return next(p for t, p in chunks(data) if t == b"VP8 ")


def frame_size(vp8: bytes) -> tuple:
    return struct.unpack("<H", vp8[6:8])[0] & 0x3FFF, struct.unpack("<H", vp8[8:10])[0] & 0x3FFF


def vp8x(vp8: bytes, flags: int = 0, canvas=None, before=(), after=()) -> bytes:
    w, h = canvas or frame_size(vp8)
    hdr = bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    return riff([(b"VP8X", hdr), *before, (b"VP8 ", vp8), *after])


def exif_blob(orientation: int = 6) -> bytes:
    ifd = struct.pack("<HHHIHH", 1, 0x0112, 3, 1, orientation, 0) + b"\0\0\0\0"
    return b"II*\0" + struct.pack("<I", 8) + ifd


XMP_TURNED = (b'<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#">'
              b'<rdf:Description xmlns:tiff="http://ns.adobe.com/tiff/1.0/" tiff:Orientation="6"/></rdf:RDF></x:xmpmeta>')


def xmp_turned_file(w: int = 40, h: int = 24, seed: int = 4) -> bytes:
    """A VP8X file whose only orientation is tiff:Orientation in an XMP chunk: Pillow's getexif() reads it from info["xmp"],
    so ImageOps.exif_transpose turns the image."""
    vp8 = vp8_of(pillow_file(content(np.random.default_rng(seed), w, h, "smooth"), 80, 4))
    return vp8x(vp8, 0x04, after=[(b"XMP ", XMP_TURNED)])


def wrapped_cases(seed: int = 1) -> list:
    """Extended-format files the decoder takes: VP8X with ICCP / EXIF / XMP chunks around the frame."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(8):
        w, h = int(rng.integers(8, 120)), int(rng.integers(8, 120))
        vp8 = vp8_of(pillow_file(content(rng, w, h, KINDS[i % 5]), int(rng.integers(10, 95)), 4))
        icc, xmp = b"\0" * (128 + i), b"<x:xmpmeta xmlns:x='adobe:ns:meta/'/>"
        variants = [vp8x(vp8), vp8x(vp8, 0x20, before=[(b"ICCP", icc)]), vp8x(vp8, 0x08, after=[(b"EXIF", exif_blob())]),
                    vp8x(vp8, 0x2C, before=[(b"ICCP", icc)], after=[(b"EXIF", exif_blob(3)), (b"XMP ", xmp)])]
        out.append((f"vp8x_{i}", variants[i % 4]))
    return out


def refused_cases(seed: int = 2) -> list:
    """[(name, bytes, expected status)] of files the decoder leaves to Pillow."""
    rng = np.random.default_rng(seed)
    a = content(rng, 40, 30, "smooth")
    lossy = pillow_file(a, 80, 4)
    vp8 = vp8_of(lossy)
    out = [("lossless", pillow_file(a, 80, 4, lossless=True), UNSUPPORTED)]
    rgba = np.concatenate([a, rng.integers(0, 256, (30, 40, 1), dtype=np.uint8)], -1)
    buf = io.BytesIO()
    Image.fromarray(rgba, "RGBA").save(buf, "WEBP", quality=80)
    out.append(("alpha", buf.getvalue(), UNSUPPORTED))
    frames = [Image.fromarray(content(rng, 32, 32, k)) for k in ("smooth", "noisy")]
    buf = io.BytesIO()
    frames[0].save(buf, "WEBP", save_all=True, append_images=frames[1:], quality=70, duration=100)
    out.append(("animated", buf.getvalue(), UNSUPPORTED))
    out.append(("truncated_half", lossy[: len(lossy) // 2], CORRUPT))
    out.append(("truncated_header", lossy[:20], CORRUPT))
    w, h = frame_size(vp8)
    out.append(("canvas_mismatch", vp8x(vp8, canvas=(w + 1, h)), UNSUPPORTED))
    inter = bytearray(vp8)
    inter[0] |= 1
    out.append(("inter_frame", riff([(b"VP8 ", bytes(inter))]), UNSUPPORTED))
    hidden = bytearray(vp8)
    hidden[0] &= ~0x10
    out.append(("show_frame_0", riff([(b"VP8 ", bytes(hidden))]), UNSUPPORTED))
    prof = bytearray(vp8)
    prof[0] = (prof[0] & ~0x0E) | (5 << 1)
    out.append(("profile_5", riff([(b"VP8 ", bytes(prof))]), UNSUPPORTED))
    out.append(("unknown_chunk", vp8x(vp8, after=[(b"ZZZZ", b"1234")]), UNSUPPORTED))
    out.append(("alpha_flag", vp8x(vp8, 0x10), UNSUPPORTED))
    big = bytearray(lossy)
    big[4:8] = struct.pack("<I", len(lossy) + 100)
    out.append(("riff_too_long", bytes(big), CORRUPT))
    giant = bytearray(vp8)                                   # 4097 x 4097: 66 049 macroblocks, over the decoder's cap
    giant[6:10] = struct.pack("<HH", 4097, 4097)
    out.append(("over_pixel_cap", riff([(b"VP8 ", bytes(giant))]), UNSUPPORTED))
    return out


# ---- libwebp's own encoder through ctypes, for what Pillow's options cannot ask for ---------------------------------------
class _Config(C.Structure):
    _fields_ = [(n, C.c_float if n in ("quality", "target_PSNR") else C.c_int) for n in (
        "lossless", "quality", "method", "image_hint", "target_size", "target_PSNR", "segments", "sns_strength",
        "filter_strength", "filter_sharpness", "filter_type", "autofilter", "alpha_compression", "alpha_filtering",
        "alpha_quality", "pass_", "show_compressed", "preprocessing", "partitions", "partition_limit", "emulate_jpeg_size",
        "thread_level", "low_memory", "near_lossless", "exact", "use_delta_palette", "use_sharp_yuv", "qmin", "qmax")]


class _Picture(C.Structure):
    _fields_ = [("use_argb", C.c_int), ("colorspace", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("y_stride", C.c_int), ("uv_stride", C.c_int),
                ("a", C.c_void_p), ("a_stride", C.c_int), ("pad1", C.c_uint32 * 2), ("argb", C.c_void_p), ("argb_stride", C.c_int),
                ("pad2", C.c_uint32 * 3), ("writer", C.c_void_p), ("custom_ptr", C.c_void_p), ("extra_info_type", C.c_int),
                ("extra_info", C.c_void_p), ("stats", C.c_void_p), ("error_code", C.c_int), ("progress_hook", C.c_void_p),
                ("user_data", C.c_void_p), ("pad3", C.c_uint32 * 3), ("pad4", C.c_void_p), ("pad5", C.c_void_p),
                ("pad6", C.c_uint32 * 8), ("memory_", C.c_void_p), ("memory_argb_", C.c_void_p), ("pad7", C.c_void_p * 2),
                ("_spare", C.c_uint8 * 256)]


class _MemWriter(C.Structure):
    _fields_ = [("mem", C.c_void_p), ("size", C.c_size_t), ("max_size", C.c_size_t), ("pad", C.c_uint32)]


_ENC_ABI = 0x020F


def load_libwebp():
    """libwebp with its encoder (and WebPDecodeYUV), or None"""
    names = [ctypes.util.find_library("webp"), "libwebp.so.7", "libwebp.so"]
    names += sorted(glob.glob(os.path.join(sys.prefix, "lib", "libwebp.so*")))
    for name in names:
        if not name:
            continue
        try:
            lib = C.CDLL(name)
            lib.WebPConfigInitInternal, lib.WebPEncode, lib.WebPDecodeYUV  # noqa: B018
            return lib
        except (OSError, AttributeError):
            continue
    return None


def libwebp_file(lib, a: np.ndarray, *, quality=75, method=4, segments=4, filter_strength=60, sharpness=0, simple=False,
                 partitions=0, sns=50) -> bytes:
    cfg = _Config()
    assert lib.WebPConfigInitInternal(C.byref(cfg), 0, C.c_float(quality), _ENC_ABI)
    cfg.method, cfg.segments, cfg.filter_strength, cfg.filter_sharpness = method, segments, filter_strength, sharpness
    cfg.filter_type, cfg.partitions, cfg.sns_strength, cfg.autofilter = 0 if simple else 1, partitions, sns, 0
    assert lib.WebPValidateConfig(C.byref(cfg))
    pic = _Picture()
    assert lib.WebPPictureInitInternal(C.byref(pic), _ENC_ABI)
    h, w = a.shape[:2]
    pic.width, pic.height = w, h
    rgb = np.ascontiguousarray(a)
    assert lib.WebPPictureImportRGB(C.byref(pic), rgb.ctypes.data_as(C.c_void_p), w * 3)
    mw = _MemWriter()
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
    """[(name, bytes)]: simple filter, filter level 0, sharpness 1..7, 2 / 4 / 8 token partitions, 1..4 segments"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = int(rng.integers(1, 160)), int(rng.integers(1, 160))
        kind = KINDS[i % len(KINDS)]
        opts = dict(quality=int(rng.integers(0, 101)), method=int(rng.integers(0, 7)), segments=1 + i % 4,
                    filter_strength=0 if i % 6 == 5 else int(rng.integers(1, 101)), sharpness=i % 8, simple=i % 3 == 1,
                    partitions=(i // 2) % 4, sns=int(rng.integers(0, 101)))
        tag = "_".join(f"{k[:4]}{int(v)}" for k, v in opts.items())
        out.append((f"enc_{i}_{kind}_{w}x{h}_{tag}", libwebp_file(lib, content(rng, w, h, kind), **opts)))
    return out


def golden_cases() -> list:
    """[(name, bytes)] of the committed files"""
    return [(os.path.basename(p), open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(GOLDEN, "*.webp")))]


def taken_cases() -> list:
    """Every case the decoder takes that needs no encoder beyond Pillow's, plus the committed ones."""
    return pillow_cases() + wrapped_cases() + golden_cases()


def damaged(data: bytes, rng, count: int) -> list:
    """Mutations of one file: bytes flipped in the headers, partition 0 and the token partitions; cuts, insertions, deletions."""
    vp8 = data.find(b"VP8 ")
    body = vp8 + 8 if vp8 >= 0 else 12
    part0 = (int.from_bytes(data[body:body + 3], "little") >> 5) if vp8 >= 0 else 0
    regions = [(0, body + 10), (body + 10, min(len(data), body + 10 + max(part0, 1))), (min(len(data) - 1, body + 10 + part0), len(data))]
    out = []
    for _ in range(count):
        b = bytearray(data)
        op = int(rng.integers(0, 6))
        if op <= 2:                                           # flips in one of the three regions
            lo, hi = regions[op]
            if hi <= lo:
                lo, hi = 0, len(b)
            for _ in range(int(rng.integers(1, 4))):
                k = int(rng.integers(lo, hi))
                b[k] ^= 1 << int(rng.integers(0, 8))
        elif op == 3:
            b = b[: int(rng.integers(1, len(b)))]
        elif op == 4:
            k = int(rng.integers(0, len(b)))
            b[k:k] = rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes()
        else:
            k = int(rng.integers(0, len(b) - 1))
            del b[k:k + int(rng.integers(1, 9))]
        out.append(bytes(b))
    return out


def pillow_rgb(data: bytes):
    """Pillow's pixels, or None where Pillow does not decode the file"""
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"))
    except Exception:
        return None


def write_golden(lib) -> None:
    """(maintenance) regenerate tests/golden/webp/ from the libwebp encoder cases"""
    os.makedirs(GOLDEN, exist_ok=True)
    for name, data in libwebp_cases(lib, n=40):
        with open(os.path.join(GOLDEN, name.split("_")[0] + "_" + name.split("_")[1] + ".webp"), "wb") as f:
            f.write(data)


if __name__ == "__main__":
    lib = load_libwebp()
    if lib is None:
        raise SystemExit("no libwebp encoder here")
    write_golden(lib)
