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

from ._views import view_signatures

DEFAULT_TOLERANCE = 48
MIN_SIDE = 8


def qualifies(width: int, height: int, box) -> bool:
    """The rule of csrc/ke_trim_core.h's ke_trim_qualifies, restated."""
    bw, bh = int(box[2]) - int(box[0]), int(box[3]) - int(box[1])
    if bw <= 0 or bh <= 0 or bw < MIN_SIDE or bh < MIN_SIDE:
        return False
    return (width - bw) * 50 >= width or (height - bh) * 50 >= height


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
    return view_signatures("trimmed", paths, tolerance, device)


__all__ = ["DEFAULT_TOLERANCE", "MIN_SIDE", "qualifies", "trimmed_signatures"]
