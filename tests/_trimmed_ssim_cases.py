"""Inputs of tests/test_trimmed_ssim_cpu.py and tests/test_gpu_trimmed_ssim.py: the shapes and boxes the luma-crop kernel is held
to, and the end-to-end corpus -- the files of _trim_cases.write_files plus one decoy per original: the original under Gaussian
noise of sigma 40 (_turned_ssim_cases.noisy), which keeps the picture's low frequencies (and so its pHash, to a few bits) and
nothing else, on a clean letterbox or white canvas.  Its content box qualifies, so the trimmed scan links it.

The seeds are picked on the CPU oracle (tests/test_trimmed_ssim_cpu.py asserts what they were picked for): every decoy's
trimmed pHash lies within the hamming threshold of, and shares a 16-bit band with, its original's stored pHash, and its box
scores under 0.5 against the original."""
from __future__ import annotations

import os

import numpy as np

import _trim_cases as T
from _turned_ssim_cases import noisy

SSIM_THRESHOLD = 0.9
# original (index into _trim_cases.originals()) -> (border kind of its decoy, s of the noise seed SEED + 700 + 10 i + s)
DECOYS = {0: ("letterbox", 1), 1: ("white margins", 0), 2: ("letterbox", 0), 5: ("white margins", 0)}
assert tuple(DECOYS) == T.FILE_ORIGINALS

# ---- the luma-crop kernel ---------------------------------------------------------------------------------------------------
KERNEL_SHAPES = ((1, 1), (7, 5), (67, 130), (257, 31), (200, 197))       # (w, h), each at 1, 3 and 4 channels
ROWS_PER_BLOCK = 32           # ke_launch_crop_luma: a workgroup of four waves for every 32 rows of the tallest box of a launch


def kernel_boxes(w: int, h: int) -> list:
    """The boxes of a w x h image: the whole image, a single pixel at each corner, and -- where the image has the room --
    boxes whose x0 and width take every residue mod 4 (with 3 channels x0 * ch then does too), the last of them from the
    second row to the last."""
    boxes = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, 0, w, 1), (0, h - 1, 1, h), (w - 1, h - 1, w, h)]
    if w >= 16 and h >= 4:
        for x0 in range(4):
            for bw in (w - 8, w - 9, w - 10, w - 11):
                boxes.append((x0, 1, x0 + bw, h if (x0, bw) == (3, w - 11) else min(h, 4 + x0)))
    return boxes


def same_band(a: int, b: int) -> bool:
    return any((a >> (16 * j)) & 0xFFFF == (b >> (16 * j)) & 0xFFFF for j in range(4))


# ---- the corpus ----------------------------------------------------------------------------------------------------------------
def decoy_picture(i: int) -> np.ndarray:
    kind, s = DECOYS[i]
    return T.bordered(noisy(T.originals()[i], T.SEED + 700 + 10 * i + s), kind)[0]


def write_corpus(folder) -> list:
    """_trim_cases.write_files' records, each with decoy = False, then one PNG per decoy (lossless: the pixels on disk are
    decoy_picture's): dict(file_id, path, original, kind, decoy), ids ascending from 1."""
    from PIL import Image

    records = [dict(r, decoy=False) for r in T.write_files(folder)]
    for i, (kind, _) in DECOYS.items():
        path = os.path.join(str(folder), f"o{i}_decoy.png")
        Image.fromarray(decoy_picture(i)).save(path)
        records.append(dict(file_id=len(records) + 1, path=path, original=i, kind=f"decoy on {kind}", decoy=True))
    return records


def families(records) -> set:
    """The groups the re-check must leave: per original the file and its bordered copies, and the drawing's two canvases."""
    groups: dict = {}
    for r in records:
        if not r["decoy"]:
            groups.setdefault(r["original"], set()).add(r["file_id"])
    return {frozenset(v) for v in groups.values()}
