"""Inputs of tests/test_gpu_turned_ssim.py: the shapes the turn kernel is held to, the pictures of the library-call tests,
and the end-to-end corpus -- three pictures, turned copies of each, and per picture one decoy: a turned copy under Gaussian
noise of sigma 40, which keeps the picture's low frequencies (and so its pHash, to a few bits) and nothing else.

The seeds are picked on the CPU oracle so that every decoy lies within the hamming threshold of, and shares a 16-bit band
with, a turned hash of its picture: ``decoy_reach`` is that check, asserted by the GPU test before it looks at any score."""
from __future__ import annotations

import os

import numpy as np

import _turned_cases as T

TILE = 64                    # KE_TURN_TILE (tests/test_turn_core_cpu.py asserts the header's value)
# (w, h): the degenerate ones, around the tile, no multiple of it, and more than three tiles each way
KERNEL_SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (67, 130), (129, 66), (257, 31),
                 (3 * TILE + 8, 3 * TILE + 5))
SEED = 20261020
SIGMA = 40.0
# the library-call tests: (a's (w, h), b's (w, h)); b is turned under every orientation
PAIR_SHAPES = (((96, 80), (80, 96)), ((96, 80), (120, 100)), ((160, 120), (120, 160)), ((40, 30), (30, 40)))
# end to end: picture -> (w, h), the orientations its true copies are made with, the orientation and noise seed of its decoy
CORPUS = (
    dict(shape=(96, 80), copies=(1, 5), decoy=6, noise=0),
    dict(shape=(160, 120), copies=(2, 6), decoy=3, noise=0),
    dict(shape=(120, 160), copies=(3, 7), decoy=4, noise=3),
)


def noisy(px: np.ndarray, seed: int, sigma: float = SIGMA) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.clip(px.astype(np.float64) + rng.normal(0.0, sigma, size=px.shape), 0, 255).astype(np.uint8)


def corpus_pictures() -> list:
    """[dict(picture, orientation, decoy, px)]: per picture the original, its copies, its decoy, in that order."""
    out = []
    for i, c in enumerate(CORPUS):
        w, h = c["shape"]
        px = T.picture(SEED + 300 + i, w, h, 3)
        out.append(dict(picture=i, orientation=0, decoy=False, px=px))
        for k in c["copies"]:
            out.append(dict(picture=i, orientation=k, decoy=False, px=T.turn_k(k, px)))
        out.append(dict(picture=i, orientation=c["decoy"], decoy=True, px=noisy(T.turn_k(c["decoy"], px), SEED + 400 + 10 * i + c["noise"])))
    return out


def write_corpus(folder) -> list:
    """The corpus as PNG files (lossless: the pixels on disk are the pixels above).  Adds file_id (from 1) and path."""
    from PIL import Image

    records = corpus_pictures()
    for n, r in enumerate(records):
        kind = "decoy" if r["decoy"] else ("copy" if r["orientation"] else "original")
        r["file_id"] = n + 1
        r["path"] = os.path.join(str(folder), f"p{r['picture']}_{kind}{r['orientation']}.png")
        Image.fromarray(r["px"]).save(r["path"])
    return records


def decoy_reach(O, records, threshold: int = T.THRESHOLD) -> dict:
    """{decoy's file_id: (other file_id, orientation, hamming)}: for every decoy the closest non-decoy file of its picture
    that the turned scan can link it to by the oracle alone -- the stored pHash of one within ``threshold`` bits of, and
    sharing a 16-bit band with, a turned hash (orientation 1..7) of the other's tile."""
    def hashes(px):
        tile = O.hash_image(px, want_tiles=True)[2]
        return [O.phash_from_tile(T.turn_k(k, tile))[0] for k in range(8)]

    table = {r["file_id"]: hashes(r["px"]) for r in records}
    out = {}
    for d in (r for r in records if r["decoy"]):
        best = None
        for o in (r for r in records if r["picture"] == d["picture"] and not r["decoy"]):
            for stored, other in ((d, o), (o, d)):
                for k in range(1, 8):
                    a, b = table[stored["file_id"]][0], table[other["file_id"]][k]
                    ham = O.hamming64(a, b)
                    if ham <= threshold and any((a >> (16 * j)) & 0xFFFF == (b >> (16 * j)) & 0xFFFF for j in range(4)):
                        if best is None or ham < best[2]:
                            best = (o["file_id"], k, ham)
        if best is not None:
            out[d["file_id"]] = best
    return out
