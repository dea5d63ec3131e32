"""Turned pHashes: the pHash of all eight orientations of a picture, for finding mirrored, flipped and rotated copies.

A capability of this library only -- the reference has no such feature.  Orientation ``k`` in 0..7 of a 2-D array ``a``::

    t = a.T if k & 4 else a
    if k & 1: t = t[:, ::-1]      # mirror, left <-> right
    if k & 2: t = t[::-1]         # flip, top <-> bottom

Turned pHash ``k`` of an image is the reference's pHash arithmetic (src/sig/phash.py:38-45) on orientation ``k`` of the
image's 32x32 LANCZOS luma tile (include/keyes.h, ``ke_hash_images_turned``); column 0 is the image's pHash.  Nothing is
written to a database: the ``signatures`` row shape is the reference's and stays.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import _native
from .formats import Offers

# orientation -> what it does to the picture; the second entry is Pillow's name for it (Image.Transpose.<name>), None for 0
ORIENTATIONS = (
    ("identity", None),
    ("mirror", "FLIP_LEFT_RIGHT"),
    ("flip", "FLIP_TOP_BOTTOM"),
    ("half turn", "ROTATE_180"),
    ("transpose", "TRANSPOSE"),
    ("quarter turn clockwise", "ROTATE_270"),
    ("quarter turn counter-clockwise", "ROTATE_90"),
    ("transverse", "TRANSVERSE"),
)
# turn(INVERSE[k], turn(k, a)) == a: the two quarter turns undo each other, every other orientation undoes itself
INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)


def turn(k: int, a: np.ndarray) -> np.ndarray:
    """Orientation ``k`` of an array whose first two axes are rows and columns (a view)."""
    if not 0 <= k < 8:
        raise ValueError(f"orientation {k} outside 0..7")
    t = np.swapaxes(a, 0, 1) if k & 4 else a
    if k & 1:
        t = t[:, ::-1]
    if k & 2:
        t = t[::-1]
    return t


def _compose_table() -> tuple:
    probe = np.arange(6).reshape(2, 3)
    views = [turn(m, probe) for m in range(8)]
    return tuple(tuple(next(m for m in range(8) if views[m].shape == turn(k, views[j]).shape and np.array_equal(views[m], turn(k, views[j])))
                       for k in range(8)) for j in range(8))


# COMPOSE[j][k] = m with turn(m, a) == turn(k, turn(j, a)): first j, then k
COMPOSE = _compose_table()


def _pillow_turned(ctx, paths: Sequence, turned: np.ndarray, ok: np.ndarray, rows: Sequence[int]) -> None:
    """The files the decoders left: ``Image.open`` in this process, then ke_hash_images_turned per channel count."""
    from PIL import Image

    from .phash import image_to_array

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
        t, status = ctx.hash_images_turned([a for _, a in items])
        idx = np.fromiter((i for i, _ in items), np.int64, len(items))
        good = status == 0
        turned[idx[good]] = t[good]
        ok[idx[good]] = True


def turned_signatures(paths: Sequence, *, device: int = 0):
    """(turned u64[n, 8], ok bool[n]) of the files at ``paths``.

    The files go kind by kind, by suffix, through the GPU decoders the hashing seam has enabled (formats.enabled_kinds:
    opt-in variables and off-switches are honoured, a follow-up decoder sees what its base left unsupported) and from there
    to ke_hash_images_turned without the pixels leaving the device.  Whatever comes back with a status other than 0, and
    every file of a suffix no decoder takes, is opened with Pillow in this process and hashed by the same call.  A file
    Pillow cannot open has ok = False and eight zeros."""
    paths = [str(p) for p in paths]
    n = len(paths)
    turned = np.zeros((n, 8), np.uint64)
    ok = np.zeros(n, bool)
    if n == 0:
        return turned, ok
    ctx = _native.get_context(device)
    at = {}
    for i, p in enumerate(paths):
        at.setdefault(p, []).append(i)
    placed: dict = {}
    offers = Offers("hash", list(at), placed)
    for kind, mine in offers:
        t, status = ctx.hash_turned(None, kind=kind, paths=mine)
        offers.ran(kind, mine, status)
        for p, row, st in zip(mine, t, status.tolist()):
            if st == 0:
                placed[p] = True
                turned[at[p]] = row
                ok[at[p]] = True
    _pillow_turned(ctx, paths, turned, ok, [i for i in range(n) if not ok[i]])
    return turned, ok


__all__ = ["ORIENTATIONS", "INVERSE", "COMPOSE", "turn", "turned_signatures"]
