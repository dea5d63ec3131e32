"""Files for the reduced-size JPEG decode and the oversize refine route, made with the installed Pillow: the grid of sizes x
sampling shapes x scan modes that the scaled decoder is held to at every scale, Pillow's pixels after a `draft` call that forces
one scale, the Image.reduce set, and the files of the whole chain against the loader."""
from __future__ import annotations

import functools
import io
import struct

import numpy as np
from PIL import Image

SIDES = tuple(range(1, 18)) + (31, 32, 33, 63, 64, 65)
SHAPES = ("444", "422", "420", "440", "gray")
SCALES = (1, 2, 4, 8)


def smooth(w: int, h: int, seed: int = 0) -> np.ndarray:
    """A smooth RGB picture (low frequencies only): at quality 90 no block comes near the IDCT bound."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(seed)
    out = np.empty((h, w, 3), np.float64)
    for c in range(3):
        fx, fy, px, py = rng.uniform(0.02, 0.2), rng.uniform(0.02, 0.2), rng.uniform(0, 6), rng.uniform(0, 6)
        out[..., c] = 128 + 70 * np.sin(xx * fx + px) * np.cos(yy * fy + py) + 40 * np.sin((xx + yy) * 0.05 + c)
    return np.clip(out, 0, 255).astype(np.uint8)


def _save(arr, **kw) -> bytes:
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **kw)
    return b.getvalue()


def as_440(data: bytes, w: int, h: int) -> bytes:
    """A 4:2:2 file of an h x w picture made into a 4:4:0 file of w x h: the luma sampling byte of the frame header set to 1 x 2
    and the two sizes exchanged.  The scan is the same bit stream -- two luma blocks, Cb, Cr per MCU, ceil(h / 16) * ceil(w / 8)
    of them either way --, the picture is scrambled, the arithmetic (block order, h1v2 upsampling) is what is compared."""
    d = bytearray(data)
    sof = max(data.find(b"\xff\xc0"), data.find(b"\xff\xc2"))
    d[sof + 5:sof + 9] = struct.pack(">HH", h, w)
    d[sof + 11] = 0x12
    return bytes(d)


def jpeg_file(w: int, h: int, shape: str, progressive: bool, seed: int = 0, **kw) -> bytes:
    kw = dict(quality=90, progressive=progressive, **kw)
    if shape == "gray":
        return _save(smooth(w, h, seed)[:, :, 1], **kw)
    if shape == "440":
        return as_440(_save(smooth(h, w, seed), subsampling=1, **kw), w, h)
    return _save(smooth(w, h, seed), subsampling={"444": 0, "422": 1, "420": 2}[shape], **kw)


def pillow_at_scale(data: bytes, scale: int):
    """(pixels, the scale libjpeg ran at) after the `draft` call that forces ``scale`` on a file with both sides >= scale."""
    with Image.open(io.BytesIO(data)) as im:
        w, h = im.size
        im.draft("RGB", (max(1, w // scale), max(1, h // scale)))
        im.load()
        return np.asarray(im), int(im.decoderconfig[0])


@functools.lru_cache(maxsize=None)
def grid():
    """[(name, file bytes)]: every shape x {sequential, progressive} at every width x height of SIDES, and one file with
    restart intervals per shape and mode."""
    out = []
    for shape in SHAPES:
        for prog in (False, True):
            for w in SIDES:
                for h in SIDES:
                    out.append((f"{shape}_p{int(prog)}_{w}x{h}", jpeg_file(w, h, shape, prog, seed=w * 131 + h)))
            out.append((f"{shape}_p{int(prog)}_restart", jpeg_file(77, 50, shape, prog, seed=5, restart_marker_blocks=3)))
    return out


@functools.lru_cache(maxsize=None)
def grid_reference():
    """{(index into grid(), scale asked for): (pixels, scale libjpeg ran at)}."""
    return {(i, s): pillow_at_scale(data, s) for i, (_, data) in enumerate(grid()) for s in SCALES}


REDUCE_PAIRS = tuple((fx, fy) for fx in range(1, 9) for fy in range(1, 9) if (fx, fy) != (1, 1)) + (      # Image.reduce((1, 1)) is a copy
    (16, 16), (9, 16), (16, 1), (1, 16), (12, 5), (3, 13), (16, 7))


def reduce_grid():
    """(w, h, fx, fy, random RGB pixels): every factor pair in 1..8 and a few up to 16, at every width and height in 1..20 --
    every partial last cell of every factor."""
    rng = np.random.default_rng(17)
    for fx, fy in REDUCE_PAIRS:
        for w in range(1, 21):
            for h in range(1, 21):
                yield w, h, fx, fy, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def reduce_cases():
    """A sample of reduce_grid() for the device, where every case is a call of its own: every factor pair, at the sizes about
    the factors and a few drawn ones."""
    rng = np.random.default_rng(7)
    for fx, fy in REDUCE_PAIRS:
        sizes = {(1, 1), (20, 20), (fx, fy), (fx + 1, fy + 1), (max(1, fx - 1), max(1, 2 * fy - 1)), (19, 7), (2 * fx, 3 * fy)}
        sizes |= {(int(rng.integers(1, 21)), int(rng.integers(1, 21))) for _ in range(3)}
        for w, h in sorted(s for s in sizes if s[0] <= 20 and s[1] <= 20):
            yield w, h, fx, fy, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


CHAIN_SIZES = ((65, 65), (128, 128), (129, 300), (255, 256), (257, 513), (511, 140), (512, 512), (520, 1030), (1100, 130), (64, 700))
CHAIN_MAX_SIDE = 64
CHAIN_FACTORS = {(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (4, 4), (5, 5), (8, 8)}


def with_orientation(data: bytes, orientation: int) -> bytes:
    """The JPEG file with an APP1 Exif segment that holds the orientation tag alone, behind SOI."""
    tiff = b"II*\x00\x08\x00\x00\x00" + struct.pack("<H", 1) + struct.pack("<HHII", 0x0112, 3, 1, orientation) + struct.pack("<I", 0)
    body = b"Exif\x00\x00" + tiff
    return data[:2] + b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body + data[2:]


def chain_files():
    """(name, suffix, file bytes) of the chain set: every size as JPEG (4:2:0, orientations 1, 3, 6, 8 in turn over the shapes
    of content) and PNG."""
    for k, (w, h) in enumerate(CHAIN_SIZES):
        for o in (1, 3, 6, 8):
            shape = ("420", "444", "422", "420")[(k + o) % 4]
            data = jpeg_file(w, h, shape, progressive=(k + o) % 3 == 0, seed=1000 + k)
            yield f"{w}x{h}_o{o}_{shape}", ".jpg", data if o == 1 else with_orientation(data, o)
        b = io.BytesIO()
        Image.fromarray(smooth(w, h, 2000 + k)).save(b, "PNG")
        yield f"{w}x{h}", ".png", b.getvalue()


def draft_scale(w: int, h: int, max_side: int) -> int:
    """The scale `im.draft("RGB", (max_side, max_side))` sets up for a w x h JPEG file (rule 1 of the loader)."""
    q = min(w // max_side, h // max_side)
    return next((s for s in (8, 4, 2) if s <= q), 1)


def thumbnail_size(w: int, h: int, box: int):
    """Image.thumbnail's target size (PIL/Image.py, preserve_aspect_ratio)."""
    import math

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    x = y = box
    aspect = w / h
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def reduce_factors(w: int, h: int, tw: int, th: int):
    """thumbnail's reducing_gap = 2.0: the box reduction in front of the resample (Image.resize)."""
    return int(w / tw / 2.0) or 1, int(h / th / 2.0) or 1
