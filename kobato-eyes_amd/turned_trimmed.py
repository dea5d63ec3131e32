"""Turned pHashes of a picture and of the picture cut to its content box, from one reading of each file: for finding copies that
are bordered AND turned -- a scan laid on the glass sideways with a white margin, a letterboxed frame that was mirrored, a framed
repost rotated a quarter turn.

A capability of this library only -- the reference has neither feature.  ``turned[i, k]`` is turned.py's turned pHash k of file
i; ``boxes[i]`` and ``has[i]`` are trimmed.py's content box and whether it qualifies; ``trimmed_turned[i, k]`` is turned pHash k
of ``im.crop(box)`` -- the pHash arithmetic on orientation k of the crop's 32 x 32 tile, so column 0 is the trimmed pHash -- and
eight zeros where the box does not qualify (include/keyes.h, ``ke_hash_images_turned_trimmed``).

The box is always found on the picture as it lies, with the reference pixel at (0, 0).  Turning does not commute with that choice
of corner: the box of a turned picture need not be the turned box.  Nothing is written to a database.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import _native
from .formats import Offers
from .trimmed import DEFAULT_TOLERANCE


def _pillow_turned_trimmed(ctx, paths: Sequence, tolerance: int, out: tuple, rows: Sequence[int]) -> None:
    """The files the decoders left: ``Image.open`` in this process, then ke_hash_images_turned_trimmed per channel count."""
    from PIL import Image

    from .phash import image_to_array

    turned, cut, boxes, has, ok = out
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
        tn, q, b, t, status = ctx.hash_images_turned_trimmed([a for _, a in items], tolerance)
        idx = np.fromiter((i for i, _ in items), np.int64, len(items))
        good = status == 0
        turned[idx[good]], cut[idx[good]], boxes[idx[good]], has[idx[good]] = tn[good], q[good], b[good], t[good]
        ok[idx[good]] = True


def turned_trimmed_signatures(paths: Sequence, *, tolerance: int = DEFAULT_TOLERANCE, device: int = 0):
    """(turned u64[n, 8], trimmed_turned u64[n, 8], boxes int32[n, 4], has bool[n], ok bool[n]) of the files at ``paths``.

    Every file is decoded once: kind by kind, by suffix, through the GPU decoders the hashing seam has enabled
    (formats.enabled_kinds) and from there to ke_hash_images_turned_trimmed without the pixels leaving the device, as
    trimmed.trimmed_signatures sends them to ke_hash_images_trimmed.  Whatever comes back with a status other than 0, and every
    file of a suffix no decoder takes, is opened with Pillow in this process and hashed by the same call.  ``has[i]``: the file's
    box qualifies and ``trimmed_turned[i]`` holds its eight hashes; otherwise they are 0 and ``boxes[i]`` still holds the box
    (four zeros: none).  A file Pillow cannot open has ok = False and zeros."""
    if not 0 <= int(tolerance) <= 255:
        raise ValueError(f"tolerance {tolerance} outside 0..255")
    paths = [str(p) for p in paths]
    n = len(paths)
    turned, cut = np.zeros((n, 8), np.uint64), np.zeros((n, 8), np.uint64)
    boxes, has, ok = np.zeros((n, 4), np.int32), np.zeros(n, bool), np.zeros(n, bool)
    if n == 0:
        return turned, cut, boxes, has, ok
    ctx = _native.get_context(device)
    at = {}
    for i, p in enumerate(paths):
        at.setdefault(p, []).append(i)
    placed: dict = {}
    offers = Offers("hash", list(at), placed)
    for kind, mine in offers:
        tn, q, b, t, status = ctx.hash_turned_trimmed(None, kind=kind, paths=mine, tolerance=int(tolerance))
        offers.ran(kind, mine, status)
        for k, (p, st) in enumerate(zip(mine, status.tolist())):
            if st == 0:
                placed[p] = True
                turned[at[p]], cut[at[p]], boxes[at[p]], has[at[p]] = tn[k], q[k], b[k], t[k]
                ok[at[p]] = True
    _pillow_turned_trimmed(ctx, paths, int(tolerance), (turned, cut, boxes, has, ok), [i for i in range(n) if not ok[i]])
    return turned, cut, boxes, has, ok


__all__ = ["turned_trimmed_signatures"]
