"""The one path from files to the hashes of their views, behind turned.turned_signatures, trimmed.trimmed_signatures and
turned_trimmed.turned_trimmed_signatures: which arrays a mode yields is _native.HASH_CALLS' row of that mode, which Context
calls make them is the table below.  A further view is a row in each.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import _native
from .formats import Offers

# mode -> (the Context call behind the GPU decoders, the one for pictures Pillow opened, whether they take ``tolerance``); each
# returns the outputs of _native.HASH_CALLS[mode] in order, then the status
CALLS = {
    "turned": ("hash_turned", "hash_images_turned", False),
    "trimmed": ("hash_trimmed", "hash_images_trimmed", True),
    "turned_trimmed": ("hash_turned_trimmed", "hash_images_turned_trimmed", True),
}


def _opened_with_pillow(paths: Sequence[str], rows: Sequence[int]) -> dict:
    """{channel count: [(row, pixels)]} of the files Pillow can open; the others are left out."""
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
    return by_ch


def view_signatures(mode: str, paths: Sequence, tolerance: int = 0, device: int = 0) -> tuple:
    """The outputs of _native.HASH_CALLS[mode] over the files at ``paths``, zeros[n, ...] each with ``has`` as bool, then ok
    bool[n].

    The files go kind by kind, by suffix, through the GPU decoders the hashing seam has enabled (formats.enabled_kinds: opt-in
    variables and off-switches are honoured, a follow-up decoder sees what its base left unsupported) and from there to the
    mode's hash call without the pixels leaving the device; a path given twice is decoded once.  Whatever comes back with a
    status other than 0, and every file of a suffix no decoder takes, is opened with Pillow in this process and hashed by the
    same call, channel count by channel count.  A file Pillow cannot open has ok = False and zeros."""
    on_device, on_host, takes_tolerance = CALLS[mode]
    keywords = {"tolerance": int(tolerance)} if takes_tolerance else {}
    paths = [str(p) for p in paths]
    n = len(paths)
    *arrays, _ = _native.hash_outputs(mode, n).values()
    ok = np.zeros(n, bool)
    if n == 0:
        return (*arrays, ok)
    ctx = _native.get_context(device)
    at: dict = {}
    for i, p in enumerate(paths):
        at.setdefault(p, []).append(i)
    placed: dict = {}
    offers = Offers("hash", list(at), placed)
    for kind, mine in offers:
        *got, status = getattr(ctx, on_device)(None, kind=kind, paths=mine, **keywords)
        offers.ran(kind, mine, status)
        taken = [j for j, st in enumerate(status.tolist()) if st == 0]
        placed.update((mine[j], True) for j in taken)
        src = [j for j in taken for _ in at[mine[j]]]                    # one assignment per array and call, not per file
        rows = [i for j in taken for i in at[mine[j]]]
        for out, new in zip(arrays, got):
            out[rows] = new[src]
        ok[rows] = True
    for items in _opened_with_pillow(paths, [i for i in range(n) if not ok[i]]).values():
        *got, status = getattr(ctx, on_host)([a for _, a in items], **keywords)
        good = status == 0
        rows = np.fromiter((i for i, _ in items), np.int64, len(items))[good]
        for out, new in zip(arrays, got):
            out[rows] = new[good]
        ok[rows] = True
    return (*arrays, ok)
