"""Inputs of tests/test_turned_cpu.py and tests/test_gpu_turned.py: orientation ``k`` of an array by the issue's definition,
the images both files use (a few low-frequency waves and a ramp with random phases over light noise: no symmetry, so that
every turned pHash lies far from the image's own), the hand-made tiles, and the files of the end-to-end test."""
from __future__ import annotations

import numpy as np

THRESHOLD = 8
# (width, height, channels) of the images ke_hash_images_turned is held to the oracle on
HASH_SHAPES = ((64, 48, 3), (97, 61, 1), (97, 61, 3), (97, 61, 4), (512, 512, 3), (512, 512, 3), (512, 512, 3),
               (1024, 512, 3), (1024, 512, 3), (3072, 40, 3), (1003, 37, 3))
# (width, height) of the pictures the end-to-end test writes as PNG and JPEG files
FILE_SHAPES = ((96, 64), (128, 96), (160, 120), (192, 128), (200, 150), (256, 192), (120, 160), (96, 128), (144, 108), (256, 144),
               (176, 132), (224, 168), (130, 97), (101, 77), (240, 180), (168, 126), (208, 156), (112, 84), (136, 102), (232, 174),
               (100, 100), (192, 192), (99, 175), (250, 96), (96, 190), (180, 135), (216, 162), (124, 93), (148, 111), (256, 128))
# planted copies: (index into FILE_SHAPES' pictures, orientation the copy is made with)
PLANTED = ((0, 1), (1, 2), (2, 3), (3, 5), (4, 6))
SEED = 20261020


def turn_k(k: int, a: np.ndarray) -> np.ndarray:
    """Orientation k of an array whose first two axes are rows and columns, as the issue defines it."""
    t = np.swapaxes(a, 0, 1) if k & 4 else a
    if k & 1:
        t = t[:, ::-1]
    if k & 2:
        t = t[::-1]
    return np.ascontiguousarray(t)


def picture(seed: int, w: int, h: int, ch: int = 3) -> np.ndarray:
    """HxW (ch = 1) or HxWxch u8: waves of 0.5 to 3 periods across the picture, a ramp, light noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / w, y / h
    planes = []
    for _ in range(3 if ch > 1 else 1):
        p = rng.uniform(-40, 40) * u + rng.uniform(-40, 40) * v
        for _ in range(6):
            fx, fy = rng.uniform(0.5, 3.0, size=2)
            p = p + rng.uniform(15, 45) * np.cos(2 * np.pi * (fx * u + rng.uniform()) ) * np.cos(2 * np.pi * (fy * v + rng.uniform()))
        planes.append(128 + p + rng.normal(0, 3, size=(h, w)))
    img = np.clip(np.stack(planes, axis=-1), 0, 255).astype(np.uint8)
    if ch == 1:
        return np.ascontiguousarray(img[:, :, 0])
    if ch == 4:
        img = np.concatenate([img, rng.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], axis=-1)
    return np.ascontiguousarray(img)


def hash_images() -> list:
    return [picture(SEED + i, w, h, ch) for i, (w, h, ch) in enumerate(HASH_SHAPES)]


def file_pictures() -> list:
    return [picture(SEED + 100 + i, w, h, 3) for i, (w, h) in enumerate(FILE_SHAPES)]


def write_files(folder) -> list:
    """The end-to-end test's files: picture i as one file (PNG for the planted pictures and every even i, JPEG of quality
    95 otherwise), then for every (i, k) of PLANTED orientation k of picture i as a PNG and as a JPEG file.  Returns
    dict(file_id, path, picture, orientation) per file, ids ascending from 1 in that order."""
    import os

    from PIL import Image

    pictures = file_pictures()
    planted = {i for i, _ in PLANTED}
    out = []

    def save(px, name, picture_index, orientation):
        path = os.path.join(str(folder), name)
        Image.fromarray(px).save(path, **({"quality": 95} if name.endswith(".jpg") else {}))
        out.append(dict(file_id=len(out) + 1, path=path, picture=picture_index, orientation=orientation))

    for i, px in enumerate(pictures):
        save(px, f"p{i:02d}.{'png' if i in planted or i % 2 == 0 else 'jpg'}", i, 0)
    for i, k in PLANTED:
        for ext in ("png", "jpg"):
            save(turn_k(k, pictures[i]), f"p{i:02d}_turned{k}.{ext}", i, k)
    return out


def tiles() -> tuple:
    """(names, 32x32 u8 tiles): random ones and the degenerate ones where an exact zero coefficient meets ``0 > mean``."""
    rng = np.random.default_rng(SEED + 7)
    names, out = [], []

    def add(name, t):
        names.append(name)
        out.append(np.ascontiguousarray(np.clip(t, 0, 255).astype(np.uint8)).reshape(32, 32))

    for i in range(25):
        add(f"random{i}", rng.integers(0, 256, size=(32, 32)))
    for i in range(4):
        add(f"smooth{i}", picture(SEED + 50 + i, 32, 32, 1))
    add("flat0", np.zeros((32, 32)))
    add("flat200", np.full((32, 32), 200))
    half = rng.integers(0, 256, size=(32, 16))
    add("lr-symmetric", np.concatenate([half, half[:, ::-1]], axis=1))
    add("tb-symmetric", np.concatenate([half.T, half.T[::-1]], axis=0))
    sq = rng.integers(0, 256, size=(32, 32))
    add("transpose-symmetric", np.triu(sq) + np.triu(sq, 1).T)
    for name, (r, c) in (("corner-tl", (0, 0)), ("corner-tr", (0, 31)), ("corner-bl", (31, 0)), ("corner-br", (31, 31))):
        t = np.zeros((32, 32))
        t[r, c] = 255
        add(name, t)
    add("ramp-h", np.tile(np.arange(32) * 8, (32, 1)))
    add("ramp-v", np.tile(np.arange(32) * 8, (32, 1)).T)
    return names, np.stack(out)


def compose(j: int, k: int) -> int:
    """The orientation m with turn_k(m, a) == turn_k(k, turn_k(j, a)) for every a."""
    probe = np.arange(6).reshape(2, 3)
    want = turn_k(k, turn_k(j, probe))
    for m in range(8):
        got = turn_k(m, probe)
        if got.shape == want.shape and np.array_equal(got, want):
            return m
    raise AssertionError((j, k))
