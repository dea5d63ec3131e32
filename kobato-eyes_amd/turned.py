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

from ._views import view_signatures

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


def turned_signatures(paths: Sequence, *, device: int = 0):
    """(turned u64[n, 8], ok bool[n]) of the files at ``paths``.

    The files go kind by kind, by suffix, through the GPU decoders the hashing seam has enabled (formats.enabled_kinds:
    opt-in variables and off-switches are honoured, a follow-up decoder sees what its base left unsupported) and from there
    to ke_hash_images_turned without the pixels leaving the device.  Whatever comes back with a status other than 0, and
    every file of a suffix no decoder takes, is opened with Pillow in this process and hashed by the same call.  A file
    Pillow cannot open has ok = False and eight zeros."""
    return view_signatures("turned", paths, device=device)


__all__ = ["ORIENTATIONS", "INVERSE", "COMPOSE", "turn", "turned_signatures"]
