"""Inputs of tests/test_turned_trimmed_cpu.py and tests/test_gpu_turned_trimmed.py: the view of a picture (a box of it, then an
orientation of that crop) on the host, the oracle's eight turned pHashes of a crop, and the end-to-end corpus:

* the files of _trim_cases.write_files (originals, bordered copies, the drawing's two canvases): orientation-0 matches;
* PLANTED: ``turn(k, bordered(original, kind))`` -- between them every border kind and every k in 1..7, PNG and JPEG of quality
  85 alternating.  Original 0 under the grey frame through JPEG is not among them: its trimmed-turned hash lies 6-8 bits from
  the original's pHash but shares no 16-bit band with it, so the banded scan cannot see it;
* the planted pictures of _turned_cases, each with its turned copy as a PNG and as a JPEG file: unboxed matches;
* one decoy per original, _trimmed_ssim_cases.decoy_picture (the original under noise of sigma 40 on a clean border), turned.

tests/test_turned_trimmed_cpu.py holds the corpus to what it is picked for, on the CPU oracle."""
from __future__ import annotations

import os

import numpy as np

import _trim_cases as T
import _trimmed_ssim_cases as S
import _turned_cases as TC
from kobato_eyes_amd import turned
from oracle import oracle as O

SSIM_THRESHOLD = S.SSIM_THRESHOLD
# (original, border kind, orientation the bordered picture is turned by, file type)
PLANTED = ((0, "letterbox", 1, "png"), (1, "white margins", 2, "jpg"), (2, "pillarbox", 3, "png"), (5, "grey frame", 4, "jpg"),
           (0, "pillarbox", 5, "jpg"), (1, "grey frame", 6, "png"), (2, "white margins", 7, "jpg"), (5, "letterbox", 5, "png"))
assert {k for _, _, k, _ in PLANTED} == set(range(1, 8)) and {kind for _, kind, _, _ in PLANTED} == set(T.BORDER_KINDS)
assert (0, "grey frame") not in {(i, kind) for i, kind, _, ext in PLANTED if ext == "jpg"}
# original -> the orientation its decoy (S.decoy_picture) is turned by
DECOY_TURNS = {0: 6, 1: 3, 2: 5, 5: 1}
assert tuple(DECOY_TURNS) == T.FILE_ORIGINALS


def view(px: np.ndarray, box, k: int) -> np.ndarray:
    """``turn(k, px[y0:y1, x0:x1])``, contiguous; ``box`` None or four zeros: the picture as it lies."""
    if box is not None and any(box):
        px = px[box[1]:box[3], box[0]:box[2]]
    return np.ascontiguousarray(turned.turn(k, px))


def pillow_view(image, box, k: int):
    """Pillow's ``crop(box).transpose(...)`` of a PIL image."""
    from PIL import Image

    out = image.crop(tuple(int(v) for v in box)) if box is not None and any(box) else image
    name = turned.ORIENTATIONS[k][1]
    return out if name is None else out.transpose(getattr(Image.Transpose, name))


def turned_hashes(px: np.ndarray) -> list:
    """The oracle's eight turned pHashes of a picture: the pHash arithmetic on every orientation of its 32 x 32 tile."""
    tile = O.hash_image(px, want_tiles=True)[2]
    return [O.phash_from_tile(TC.turn_k(k, tile))[0] for k in range(8)]


def trimmed_turned_hashes(px: np.ndarray, tol: int = T.TOLERANCE):
    """(box, the eight turned pHashes of the crop or None where the box does not qualify), the box found on ``px`` as it lies."""
    box = T.content_box(px, tol)
    if not T.qualifies(px.shape[1], px.shape[0], box):
        return box, None
    return box, turned_hashes(T.crop(px, box))


def planted_picture(n: int) -> np.ndarray:
    i, kind, k, _ = PLANTED[n]
    return TC.turn_k(k, T.bordered(T.originals()[i], kind)[0])


def decoy_picture(i: int) -> np.ndarray:
    return TC.turn_k(DECOY_TURNS[i], S.decoy_picture(i))


def write_corpus(folder) -> list:
    """dict(file_id, path, family, orientation, kind, decoy, planted) per file, ids ascending from 1.  ``family``: what the file
    is a copy of -- ("trim", original), ("trim", "drawing") or ("turn", picture); ``orientation``: what the file's picture was
    turned by after it got its border (0: not turned); ``planted``: one of PLANTED, bordered and turned."""
    from PIL import Image

    out = [dict(file_id=r["file_id"], path=r["path"], family=("trim", r["original"]), orientation=0, kind=r["kind"], decoy=False, planted=False)
           for r in T.write_files(folder)]

    def save(px, name, **facts):
        path = os.path.join(str(folder), name)
        Image.fromarray(px).save(path, **({"quality": 85} if name.endswith(".jpg") else {}))
        out.append(dict(file_id=len(out) + 1, path=path, **facts))

    for n, (i, kind, k, ext) in enumerate(PLANTED):
        save(planted_picture(n), f"o{i}_{kind.replace(' ', '_')}_turned{k}.{ext}", family=("trim", i), orientation=k, kind=kind, decoy=False,
             planted=True)
    pictures = TC.file_pictures()
    for i, k in TC.PLANTED:
        save(pictures[i], f"p{i:02d}.png", family=("turn", i), orientation=0, kind=None, decoy=False, planted=False)
        for ext in ("png", "jpg"):
            save(TC.turn_k(k, pictures[i]), f"p{i:02d}_turned{k}.{ext}", family=("turn", i), orientation=k, kind=None, decoy=False, planted=False)
    for i, k in DECOY_TURNS.items():
        save(decoy_picture(i), f"o{i}_decoy_turned{k}.png", family=("trim", i), orientation=k, kind=f"decoy on {S.DECOYS[i][0]}", decoy=True,
             planted=False)
    return out


def families(records) -> set:
    """The groups the re-check must leave: the files of a family, decoys left out."""
    groups: dict = {}
    for r in records:
        if not r["decoy"]:
            groups.setdefault(r["family"], set()).add(r["file_id"])
    return {frozenset(v) for v in groups.values()}


def original_of(records) -> dict:
    """family -> file_id of its unturned, unbordered file."""
    return {r["family"]: r["file_id"] for r in records if r["kind"] is None and r["orientation"] == 0 and r["family"][1] != "drawing"}
