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

from ._views import view_signatures
from .trimmed import DEFAULT_TOLERANCE


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
    return view_signatures("turned_trimmed", paths, tolerance, device)


__all__ = ["turned_trimmed_signatures"]
