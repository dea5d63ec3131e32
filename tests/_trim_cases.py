"""Inputs of the trimmed-duplicates tests (test_trim_core_cpu.py, test_trimmed_cpu.py, test_gpu_trimmed.py): the content box
by the issue's definition in NumPy and by its Pillow recipe, the qualifying rule restated, pictures with a known placed
rectangle and border colour, the shape grid of the box kernel, and the files of the end-to-end test."""
from __future__ import annotations

import io

import numpy as np

import _scan_standin
from _turned_cases import picture

THRESHOLD = 8
TOLERANCE = 48
TOLERANCES = (0, 1, 48, 254, 255)
SEED = 20261021
# widths whose 3-channel rows cross the 16-byte vectors at every phase, beside 1..9
WIDE = (5, 6, 21, 22, 43)


# ---- the definition -----------------------------------------------------------------------------------------------------
def content_box(px: np.ndarray, tol: int) -> tuple:
    """(x0, y0, x1, y1) by the definition; four zeros when no pixel differs.  The fourth channel is ignored."""
    a = (px if px.ndim == 3 else px[:, :, None])[:, :, :3].astype(np.int16)
    differs = np.abs(a - a[0, 0]).max(axis=2) > tol
    if not differs.any():
        return (0, 0, 0, 0)
    ys, xs = np.nonzero(differs.any(axis=1))[0], np.nonzero(differs.any(axis=0))[0]
    return (int(xs[0]), int(ys[0]), int(xs[-1]) + 1, int(ys[-1]) + 1)


def pillow_box(px: np.ndarray, tol: int) -> tuple:
    """The issue's Pillow recipe (RGBA first through convert("RGB"))."""
    from PIL import Image, ImageChops

    im = Image.fromarray(px)
    if im.mode == "RGBA":
        im = im.convert("RGB")
    bg = Image.new(im.mode, im.size, im.getpixel((0, 0)))
    mask = ImageChops.difference(im, bg).point(lambda v: 255 if v > tol else 0)
    box = mask.getbbox()
    return (0, 0, 0, 0) if box is None else tuple(box)


def qualifies(w: int, h: int, box) -> bool:
    """The qualifying rule, restated from the issue."""
    bw, bh = box[2] - box[0], box[3] - box[1]
    if bw <= 0 or bh <= 0:
        return False
    if bw < 8 or bh < 8:
        return False
    return (w - bw) * 50 >= w or (h - bh) * 50 >= h


def crop(px: np.ndarray, box) -> np.ndarray:
    return np.ascontiguousarray(px[box[1]:box[3], box[0]:box[2]])


# ---- the box kernel's grid ----------------------------------------------------------------------------------------------
def grid_shapes(band: int) -> list:
    """(w, h): every shape 1..9 x 1..9, the wide widths, the heights round the band."""
    widths = sorted(set(range(1, 10)) | set(WIDE))
    heights = sorted(set(range(1, 10)) | {band - 1, band, band + 1, 2 * band + 3})
    return [(w, h) for w in widths for h in heights]


def grid_picture(rng, w: int, h: int, ch: int) -> np.ndarray:
    """A corner colour with +-1 of noise everywhere, and inside a random rectangle a third of the bytes random: boxes of every
    position, and values on both sides of every tolerance."""
    bg = rng.integers(0, 256, size=ch)
    px = np.clip(bg + rng.integers(-1, 2, size=(h, w, ch)), 0, 255).astype(np.uint8)
    x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
    x1, y1 = int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1))
    inside = rng.integers(0, 256, size=(y1 - y0, x1 - x0, ch), dtype=np.uint8)
    keep = rng.integers(0, 3, size=inside.shape) != 0
    px[y0:y1, x0:x1] = np.where(keep, px[y0:y1, x0:x1], inside)
    return np.ascontiguousarray(px[:, :, 0] if ch == 1 else px)


def single_pixel_cases(ch: int, tol: int) -> list:
    """(name, picture, box): one differing pixel in each corner and on each edge of a 23 x 11 picture; a pixel that differs in
    exactly one channel by tol (no box) and by tol + 1; for 4 channels a picture that differs only in its fourth byte."""
    w, h = 23, 11
    base = np.zeros((h, w, ch), np.uint8)
    out = []
    for name, (x, y) in (("top-left", (0, 0)), ("top-right", (w - 1, 0)), ("bottom-left", (0, h - 1)), ("bottom-right", (w - 1, h - 1)),
                         ("top", (9, 0)), ("bottom", (9, h - 1)), ("left", (0, 5)), ("right", (w - 1, 5)), ("inside", (9, 5))):
        if (x, y) == (0, 0):
            continue                                     # the corner pixel is the reference: it cannot differ from itself
        px = base.copy()
        px[y, x, :min(ch, 3)] = min(tol + 1, 255)
        out.append((name, px, (x, y, x + 1, y + 1) if tol < 255 else (0, 0, 0, 0)))
    for c in range(min(ch, 3)):
        px = base.copy()
        px[4, 7, c] = tol
        out.append((f"channel {c} by tol", px, (0, 0, 0, 0)))
        if tol < 255:
            px = base.copy()
            px[4, 7, c] = tol + 1
            out.append((f"channel {c} by tol + 1", px, (7, 4, 8, 5)))
    if ch == 4:
        px = base.copy()
        px[:, :, 3] = np.arange(w * h, dtype=np.uint8).reshape(h, w)
        out.append(("fourth byte only", px, (0, 0, 0, 0)))
    return [(n, np.ascontiguousarray(p[:, :, 0] if ch == 1 else p), b) for n, p, b in out]


# ---- pictures with a placed rectangle -------------------------------------------------------------------------------------
def place(content: np.ndarray, canvas_w: int, canvas_h: int, x: int, y: int, colour, tol: int = TOLERANCE) -> np.ndarray:
    """``content`` (h x w x 3) at (x, y) of a canvas of ``colour``.  Asserts what makes the definition alone yield the placed
    rectangle on this lossless picture: every outermost row and column of the content holds a pixel farther than ``tol``
    from the border colour, and the pixel at the image corner is border, not content."""
    h, w = content.shape[:2]
    assert 0 <= x and x + w <= canvas_w and 0 <= y and y + h <= canvas_h
    assert x > 0 or y > 0, "the content's own pixel at the image corner would be the reference"
    colour = np.asarray(colour, np.int16)
    far = np.abs(content.astype(np.int16) - colour).max(axis=2) > tol
    assert far[0].any() and far[-1].any() and far[:, 0].any() and far[:, -1].any(), "an outermost row or column melts into the border"
    canvas = np.empty((canvas_h, canvas_w, 3), np.uint8)
    canvas[:] = colour.astype(np.uint8)
    canvas[y:y + h, x:x + w] = content
    assert content_box(canvas, tol) == (x, y, x + w, y + h)
    return canvas


# the border kinds of the issue: name -> (canvas size, position, colour) of a w x h content
BORDER_KINDS = {
    "letterbox": lambda w, h: ((w, h + 2 * (h // 6)), (0, h // 6), (0, 0, 0)),
    "white margins": lambda w, h: ((w + w // 10 + w // 4, h + h // 7 + h // 12), (w // 10, h // 7), (255, 255, 255)),
    "pillarbox": lambda w, h: ((w + 2 * (w // 5), h), (w // 5, 0), (0, 0, 0)),
    "grey frame": lambda w, h: ((w + 18, h + 18), (9, 9), (48, 48, 48)),
}
# (width, height) of the originals of the CPU probe and of the end-to-end test: 97 x 64 up to 256 px
ORIGINAL_SHAPES = ((97, 64), (128, 96), (160, 120), (200, 150), (256, 144), (120, 160))
FILE_ORIGINALS = (0, 1, 2, 5)      # the originals the end-to-end test writes: no bordered copy of these exceeds 256 px


def originals() -> list:
    return [picture(SEED + i, w, h, 3) for i, (w, h) in enumerate(ORIGINAL_SHAPES)]


def bordered(content: np.ndarray, kind: str) -> tuple:
    """(picture, placed box) of ``content`` under a border kind."""
    h, w = content.shape[:2]
    (cw, chh), (x, y), colour = BORDER_KINDS[kind](w, h)
    return place(content, cw, chh, x, y, colour), (x, y, x + w, y + h)


def through_jpeg(px: np.ndarray, quality: int = 85) -> np.ndarray:
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", quality=quality)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


def drawing(seed: int, w: int, h: int) -> np.ndarray:
    """Dark strokes on white that reach all four sides of their w x h rectangle."""
    rng = np.random.default_rng(seed)
    px = np.full((h, w, 3), 255, np.uint8)
    for _ in range(14):
        x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
        px[y0:y0 + int(rng.integers(3, h // 2)), x0:x0 + int(rng.integers(3, 9))] = rng.integers(0, 120, size=3)
        px[y0:y0 + int(rng.integers(3, 9)), x0:x0 + int(rng.integers(3, w // 2))] = rng.integers(0, 120, size=3)
    px[0, 3:w // 2] = 20
    px[-1, w // 3:] = 30
    px[2:h // 2, 0] = 40
    px[h // 4:, -1] = 50
    return px


def write_files(folder) -> list:
    """The end-to-end test's files: every original as a PNG; of every original one copy per border kind, PNG and JPEG (quality
    85) alternating; one drawing on two different white canvases (PNG).  Returns dict(file_id, path, original, kind) per file,
    ids ascending from 1; the drawing's files have original = "drawing"."""
    import os

    from PIL import Image

    out = []

    def save(px, name, original, kind):
        path = os.path.join(str(folder), name)
        Image.fromarray(px).save(path, **({"quality": 85} if name.endswith(".jpg") else {}))
        out.append(dict(file_id=len(out) + 1, path=path, original=original, kind=kind))

    pictures = [(i, originals()[i]) for i in FILE_ORIGINALS]
    for i, px in pictures:
        save(px, f"o{i}.png", i, None)
    for i, px in pictures:
        for k, kind in enumerate(BORDER_KINDS):
            save(bordered(px, kind)[0], f"o{i}_{kind.replace(' ', '_')}.{'png' if (i + k) % 2 == 0 else 'jpg'}", i, kind)
    d = drawing(SEED + 50, 150, 110)
    save(place(d, 256, 200, 60, 20, (255, 255, 255)), "drawing_canvas_a.png", "drawing", "canvas a")
    save(place(d, 190, 256, 11, 97, (255, 255, 255)), "drawing_canvas_b.png", "drawing", "canvas b")
    return out


# ---- the scan of trimmed_edges, by the oracle ----------------------------------------------------------------------------------
class OracleScanContext(_scan_standin.OracleScanContext):
    """The shared stand-in, held to the scan from first_new: trimmed_edges must not ask for the cross scan."""

    def hamming_scan(self, hashes, n, *, cross=False, **keywords):
        assert not cross
        return super().hamming_scan(hashes, n, cross=cross, **keywords)
