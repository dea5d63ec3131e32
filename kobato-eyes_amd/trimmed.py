"""Trimmed pHashes: the pHash of a picture cut to its content box, for finding the same picture with a margin round it -- a
letterboxed or pillarboxed screenshot, a scan on a white page, a drawing on a larger canvas, a framed repost.

A capability of this library only -- the reference has no such feature.  The definition (include/keyes.h)::

    ref  = pixel (0, 0);  a pixel differs when max over c of |p[c] - ref[c]| > tolerance  (the fourth byte ignored)
    box  = (x0, y0, x1, y1): smallest x and y of a differing pixel, largest plus one; none when no pixel differs

which is Pillow's ``ImageChops.difference(im, Image.new(im.mode, im.size, im.getpixel((0, 0)))).point(lambda v: 255 if v >
tol else 0).getbbox()``.  A box qualifies (``qualifies``) when it exists, both sides are >= 8 and it cuts at least 2 % off
one axis; the trimmed pHash is the pHash of ``im.crop(box)``.  Nothing is written to a database.

The default tolerance of 48 rests on synthetic pictures and a stand-in DCT: the smallest of 16, 32, 48, 64
that kept JPEG copies of four border kinds within the scan's threshold of 8.  A larger one eats more dark content beside a
black bar.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import _native
from .formats import Offers

DEFAULT_TOLERANCE = 48
MIN_SIDE = 8


def qualifies(width: int, height: int, box) -> bool:
    """The rule of csrc/ke_trim_core.h's ke_trim_qualifies, restated."""
    bw, bh = int(box[2]) - int(box[0]), int(box[3]) - int(box[1])
    if bw <= 0 or bh <= 0 or bw < MIN_SIDE or bh < MIN_SIDE:
        return False
    return (width - bw) * 50 >= width or (height - bh) * 50 >= height


def _pillow_trimmed(ctx, paths: Sequence, tolerance: int, out: tuple, rows: Sequence[int]) -> None:
    """The files the decoders left: ``Image.open`` in this process, then ke_hash_images_trimmed per channel count."""
    from PIL import Image

    from .phash import image_to_array

    hashes, boxes, has, ok = out
    by_ch: dict = {}
    for i in rows:
        try:
            with Image.open(paths[i]) as im:
                arr = image_to_array(im)
        except Exception:  # noqa: BLE001 - whatever Pillow raises for a file it cannot open: the file is not ok
            continue
        if arr.shape[0] > 0 and arr.shape[1] > 0:
            by_ch.setdefault(1 if arr.ndim == 2 else arr.shape[2], []).append((i, arr))
    for items in by_ch.values():
        ph, b, t, status = ctx.hash_images_trimmed([a for _, a in items], tolerance)
        idx = np.fromiter((i for i, _ in items), np.int64, len(items))
        good = status == 0
        hashes[idx[good]], boxes[idx[good]], has[idx[good]] = ph[good], b[good], t[good]
        ok[idx[good]] = True


def trimmed_signatures(paths: Sequence, *, tolerance: int = DEFAULT_TOLERANCE, device: int = 0):
    """(hashes u64[n], boxes int32[n, 4], has bool[n], ok bool[n]) of the files at ``paths``.

    The files go kind by kind, by suffix, through the GPU decoders the hashing seam has enabled (formats.enabled_kinds) and
    from there to ke_hash_images_trimmed without the pixels leaving the device, as turned.turned_signatures sends them to
    ke_hash_images_turned.  Whatever comes back with a status other than 0, and every file of a suffix no decoder takes, is
    opened with Pillow in this process and hashed by the same call.  ``has[i]``: the file's box qualifies and ``hashes[i]``
    is its trimmed pHash; otherwise the hash is 0 and ``boxes[i]`` still holds the box (four zeros: none).  A file Pillow
    cannot open has ok = False and zeros."""
    if not 0 <= int(tolerance) <= 255:
        raise ValueError(f"tolerance {tolerance} outside 0..255")
    paths = [str(p) for p in paths]
    n = len(paths)
    hashes, boxes = np.zeros(n, np.uint64), np.zeros((n, 4), np.int32)
    has, ok = np.zeros(n, bool), np.zeros(n, bool)
    if n == 0:
        return hashes, boxes, has, ok
    ctx = _native.get_context(device)
    at = {}
    for i, p in enumerate(paths):
        at.setdefault(p, []).append(i)
    placed: dict = {}
    offers = Offers("hash", list(at), placed)
    for kind, mine in offers:
        ph, b, t, status = ctx.hash_trimmed(None, kind=kind, paths=mine, tolerance=int(tolerance))
        offers.ran(kind, mine, status)
        for k, (p, st) in enumerate(zip(mine, status.tolist())):
            if st == 0:
                placed[p] = True
                hashes[at[p]], boxes[at[p]], has[at[p]] = ph[k], b[k], t[k]
                ok[at[p]] = True
    _pillow_trimmed(ctx, paths, int(tolerance), (hashes, boxes, has, ok), [i for i in range(n) if not ok[i]])
    return hashes, boxes, has, ok


__all__ = ["DEFAULT_TOLERANCE", "MIN_SIDE", "qualifies", "trimmed_signatures"]
