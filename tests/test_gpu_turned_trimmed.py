"""Copies that are both bordered and turned, on the device.

1. ke_crop_turn_luma over one mixed batch == turn(k, O.luma(px)[y0:y1, x0:x1]) byte for byte, guard bytes round every plane
   untouched; on whole pictures it is ke_turn_luma; what it refuses.
2. ke_ssim_pairs_viewed(a, b, box_a, box_b, orient_b) is bit-equal (float64 ==, same status) to ke_ssim_pairs on host-made
   turn(k, crop)s: luma is per pixel, the turn a permutation and every resample plan pinned bit-exact, so there is no tolerance.
   With no orientation it is ke_ssim_pairs_boxed, with no box ke_ssim_pairs_turned; the four pair calls in any order on one
   context answer alike.  Against the oracle's ssim_fit of the views:
   1e-5 in the default mode, 1e-6 in the exact one -- the bars of tests/test_gpu_parity.py.
3. ke_hash_images_turned_trimmed: its columns are ke_hash_images_turned's and ke_hash_images_trimmed's, and the turned hashes of
   the crop are the oracle's, at 1, 3 and 4 channels, host and device pixels, in a ragged batch.
4. refine_turned_trimmed_pairs at the seam: PNG and JPEG files, == refine_pairs on files that hold Pillow's
   crop(box).transpose(...); flags off; a PPM file, a missing file, a flat picture, the stats.
5. find_turned_trimmed_duplicates and scan-dups --turned-trimmed on _turned_trimmed_cases' corpus
   (tests/test_turned_trimmed_cpu.py holds the corpus to what it is picked for)."""
from __future__ import annotations

import csv
import os
import sqlite3
from pathlib import Path

import numpy as np
import pytest

import _trim_cases as T
import _trimmed_ssim_cases as S
import _turned_cases as TC
import _turned_ssim_cases as TS
import _turned_trimmed_cases as V
import kobato_eyes_amd as K
from kobato_eyes_amd import _native, api, cli, refine, turned
from kobato_eyes_amd.scanner import DuplicateFile
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _native.get_context(0)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
BEHIND, FRONT = 16, 3
TILE_SIDES = (63, 64, 65, 128, 129)


def _kernel_boxes(w: int, h: int) -> list:
    """_trimmed_ssim_cases.kernel_boxes, and on the two large shapes boxes whose sides lie round one and two tiles: every
    (bw, bh) of TILE_SIDES that fits 200 x 197; on 257 x 31, where no such height fits, those widths at a height of 29."""
    boxes = list(S.kernel_boxes(w, h))
    if (w, h) == (200, 197):
        boxes += [((bw + bh) % 4, (bw + 2 * bh) % 3, (bw + bh) % 4 + bw, (bw + 2 * bh) % 3 + bh) for bw in TILE_SIDES for bh in TILE_SIDES]
    if (w, h) == (257, 31):
        boxes += [(bw % 5, 1, bw % 5 + bw, 30) for bw in TILE_SIDES]
    assert all(0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h for x0, y0, x1, y1 in boxes)
    return boxes


def test_crop_turn_luma_on_a_mixed_batch(ctx):
    rng = np.random.default_rng(T.SEED + 900)
    sources, src_off, at = [], [], 0
    for w, h in S.KERNEL_SHAPES:                        # packed back to back: a 1 x 1 grey image puts the rest off the dwords
        for ch in (1, 3, 4):
            px = rng.integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
            sources.append(px)
            src_off.append(at)
            at += px.size
    assert {o % 4 for o in src_off} == {0, 1, 2, 3}
    flat = np.concatenate([px.reshape(-1) for px in sources])
    chans = [1 if px.ndim == 2 else px.shape[2] for px in sources]
    jobs = [(i, box, k) for k in range(8) for i, px in enumerate(sources) for box in _kernel_boxes(px.shape[1], px.shape[0])]
    lumas = [O.luma(px) for px in sources]
    want = [V.view(lumas[i], box, k) for i, box, k in jobs]
    dst_off, at = [], FRONT                                          # planes packed too, 16 guard bytes behind each
    for p in want:
        dst_off.append(at)
        at += p.size + BEHIND
    total = at
    # what the batch is made to hold: every residue mod 4 of the box's first source byte, of both sides of the box and of the
    # plane's address, under every orientation; the first and the last byte of every image as a box of one pixel; boxes of more
    # than one tile each way
    for k in range(8):
        mine = [(i, box, o) for (i, box, kk), o in zip(jobs, dst_off) if kk == k]
        assert {(src_off[i] + box[0] * chans[i]) % 4 for i, box, _ in mine} == {0, 1, 2, 3}
        assert {(box[2] - box[0]) % 4 for _, box, _ in mine} == {0, 1, 2, 3} == {(box[3] - box[1]) % 4 for _, box, _ in mine}
        assert {o % 4 for _, _, o in mine} == {0, 1, 2, 3}
    for i, px in enumerate(sources):
        h, w = px.shape[:2]
        assert all((i, b, k) in jobs for b in ((0, 0, 1, 1), (w - 1, h - 1, w, h), (0, 0, w, h)) for k in range(8))
    assert sum(box[2] - box[0] > 128 and box[3] - box[1] > 128 for _, box, _ in jobs) >= 8
    src, dst = ctx.malloc(flat.nbytes), ctx.malloc(total)
    try:
        assert src % 4 == 0 and dst % 4 == 0
        ctx.memcpy(src, flat, flat.nbytes)
        ctx.memcpy(dst, np.full(total, 0xA5, np.uint8), total)
        ctx.crop_turn_luma(src, [src_off[i] for i, _, _ in jobs], [sources[i].shape[1] for i, _, _ in jobs],
                           [sources[i].shape[0] for i, _, _ in jobs], [chans[i] for i, _, _ in jobs], [box for _, box, _ in jobs],
                           [k for _, _, k in jobs], dst, dst_off)
        assert ctx.last_kernel_ms(8) >= 0.0
        got = np.empty(total, np.uint8)
        ctx.memcpy(got, dst, total)
    finally:
        ctx.free(src)
        ctx.free(dst)
    assert np.all(got[:FRONT] == 0xA5)
    for (i, box, k), p, o in zip(jobs, want, dst_off):
        assert np.array_equal(got[o:o + p.size].reshape(p.shape), p), (sources[i].shape, box, k)
        assert np.all(got[o + p.size:o + p.size + BEHIND] == 0xA5) and np.all(got[o - FRONT:o] == 0xA5), (sources[i].shape, box, k)


def test_crop_turn_luma_of_the_whole_picture_is_turn_luma(ctx):
    """One kernel behind both calls: the box (0, 0, w, h) of every shape of _turned_ssim_cases.KERNEL_SHAPES at 1, 3 and 4
    channels under every orientation is ke_turn_luma's plane byte for byte, the guard bytes round every plane untouched."""
    rng = np.random.default_rng(T.SEED + 901)
    sources = [rng.integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8) for w, h in TS.KERNEL_SHAPES for ch in (1, 3, 4)]
    src_off = np.concatenate([[0], np.cumsum([px.size for px in sources])[:-1]]).tolist()      # packed back to back: off the dwords
    assert {o % 4 for o in src_off} == {0, 1, 2, 3}
    flat = np.concatenate([px.reshape(-1) for px in sources])
    jobs = [(i, k) for k in range(8) for i in range(len(sources))]
    dst_off, at = [], FRONT
    for i, _ in jobs:
        dst_off.append(at)
        at += sources[i].shape[0] * sources[i].shape[1] + BEHIND
    total = at
    widths, heights = [sources[i].shape[1] for i, _ in jobs], [sources[i].shape[0] for i, _ in jobs]
    chans = [1 if sources[i].ndim == 2 else sources[i].shape[2] for i, _ in jobs]
    where = ([src_off[i] for i, _ in jobs], widths, heights, chans)
    src, dst = ctx.malloc(flat.nbytes), ctx.malloc(total)
    got = []
    try:
        ctx.memcpy(src, flat, flat.nbytes)
        for boxed in (False, True):
            ctx.memcpy(dst, np.full(total, 0xA5, np.uint8), total)
            if boxed:
                ctx.crop_turn_luma(src, *where, [(0, 0, w, h) for w, h in zip(widths, heights)], [k for _, k in jobs], dst, dst_off)
            else:
                ctx.turn_luma(src, *where, [k for _, k in jobs], dst, dst_off)
            got.append(np.empty(total, np.uint8))
            ctx.memcpy(got[-1], dst, total)
    finally:
        ctx.free(src)
        ctx.free(dst)
    assert np.array_equal(got[0], got[1])
    lumas = [O.luma(px) for px in sources]
    assert np.all(got[1][:FRONT] == 0xA5)
    for (i, k), o in zip(jobs, dst_off):
        p = np.ascontiguousarray(turned.turn(k, lumas[i]))
        assert np.array_equal(got[1][o:o + p.size].reshape(p.shape), p), (sources[i].shape, k)
        assert np.all(got[1][o + p.size:o + p.size + BEHIND] == 0xA5), (sources[i].shape, k)


def test_crop_turn_luma_refuses_what_it_cannot_take(ctx):
    dev = ctx.malloc(256)
    try:
        for w, h, ch, box, k in ((6, 5, 3, (2, 1, 2, 4), 1), (6, 5, 3, (0, 3, 4, 3), 1), (6, 5, 3, (0, 0, 7, 5), 4), (6, 5, 3, (0, 0, 6, 6), 4),
                                 (6, 5, 3, (-1, 0, 3, 3), 2), (6, 5, 2, (0, 0, 3, 3), 2), (0, 5, 3, (0, 0, 1, 1), 0), (6, 5, 3, (0, 0, 3, 3), 8),
                                 (6, 5, 3, (0, 0, 3, 3), -1)):
            with pytest.raises(ValueError):
                ctx.crop_turn_luma(dev, [0], [w], [h], [ch], [box], [k], dev + 128, [0])
        ctx.crop_turn_luma(dev, [], [], [], [], np.zeros((0, 4), np.int32), [], dev, [])     # nothing to do is no error
    finally:
        ctx.free(dev)


# ---- 2. the library call ---------------------------------------------------------------------------------------------------------
def _boxes_of(w: int, h: int) -> tuple:
    """Two boxes of a w x h picture (both even): margins of different sizes on every side; a cut off the left and the right alone.
    Every corner is even, so that every view and every common size of the calls below has an area that is a multiple of four --
    see test_ssim_pairs_viewed_is_ssim_pairs_on_the_host_made_views."""
    return (2 * (w // 16) + 2, 2 * (h // 20), w - 2 * (w // 12), h - 2 * (h // 24) - 2), (4, 0, w - 6, h)


def _odd_boxes_of(w: int, h: int) -> tuple:
    """The same with odd margins: views and common sizes of odd areas."""
    return (w // 8 + 1, h // 10, w - w // 6, h - h // 12 - 1), (3, 0, w - 5, h)


def _images() -> list:
    images = []
    for n, (sa, sb) in enumerate(TS.PAIR_SHAPES):
        a = TC.picture(TS.SEED + 600 + n, sa[0], sa[1], 3)
        b = TS.noisy(TC.picture(TS.SEED + 600 + n, sb[0], sb[1], 3), TS.SEED + 650 + n, 6.0)
        images += [a, b]
    return images


def _rows(boxes_of) -> list:
    """(a, b, box_a, box_b, k), None for the image as it lies: over the four pairs every k with a box on a only, on b only and on
    both, a row per pair with its sides exchanged, and one (image, box) under two orientations in one call."""
    rows = []
    for n, (sa, sb) in enumerate(TS.PAIR_SHAPES):
        (a1, a2), (b1, b2) = boxes_of(*sa), boxes_of(*sb)
        for k in range(8):
            rows.append(((2 * n, 2 * n + 1, a1, None, k), (2 * n, 2 * n + 1, None, b1, k), (2 * n, 2 * n + 1, a2, b2, k))[(n + k) % 3])
        rows += [(2 * n + 1, 2 * n, b2, a1, 5), (2 * n, 2 * n + 1, a2, b1, 6), (2 * n, 2 * n + 1, a2, b1, 3)]
    rows.append((0, 0, boxes_of(96, 80)[0], boxes_of(96, 80)[1], 7))                     # one image against itself, boxed two ways
    for k in range(8):
        assert {(r[2] is None, r[3] is None) for r in rows if r[4] == k} >= {(False, True), (True, False), (False, False)}, k
    return rows


@pytest.fixture(scope="module")
def pairs():
    """The images of _turned_ssim_cases.PAIR_SHAPES (a_0, b_0, a_1, b_1, ...), the rows of _rows, the host-made views and the
    oracle's scores: made once."""
    images, rows = _images(), _rows(_boxes_of)
    views = [(V.view(images[a], ba, 0), V.view(images[b], bb, k)) for a, b, ba, bb, k in rows]
    assert all(v.shape[0] % 2 == 0 and v.shape[1] % 2 == 0 for two in views for v in two)
    oracle = [O.ssim_fit(va, vb) for va, vb in views]
    return dict(images=images, rows=rows, views=views, oracle=oracle)


def _columns(rows) -> tuple:
    zero = (0, 0, 0, 0)
    return ([r[0] for r in rows], [r[1] for r in rows], [r[2] or zero for r in rows], [r[3] or zero for r in rows], [r[4] for r in rows])


def test_ssim_pairs_viewed_is_ssim_pairs_on_the_host_made_views(ctx, pairs):
    rows = pairs["rows"]
    got, status = ctx.ssim_pairs_viewed(pairs["images"], *_columns(rows))
    flat = [v for two in pairs["views"] for v in two]
    want, want_status = ctx.ssim_pairs(flat, list(range(0, len(flat), 2)), list(range(1, len(flat), 2)))
    for row, g, w, gs, ws in zip(rows, got.tolist(), want.tolist(), status.tolist(), want_status.tolist()):
        print(row, g, w)
        assert gs == ws == 0 and g == w, row
    assert len(set(got.tolist())) > len(rows) // 2                                       # the views change the scores: not all alike


def test_ssim_pairs_viewed_on_views_of_odd_areas(ctx):
    """Why the boxes of the test above are even.  The SSIM kernel (ke_ssim.hip, untouched here) reads a plane's last dword whole,
    so where a plane of the fitted stack does not end on a dword it sees up to three bytes of what lies behind it -- the next
    plane of the call -- in columns it masks out; a masked column shares one reciprocal with up to three scored ones, so those
    bytes can move the last bits of a few quotients of the plane's last row.  Two calls that stack their planes differently --
    this one makes a shared (image, box, orientation) once, ke_ssim_pairs on host-made views gets every view as an image of its
    own -- then agree bit for bit only where every plane's area is a multiple of four.  Elsewhere the planes are still equal
    byte for byte, and the scores differ by at most that: the two groups of four quotients at the ends of the last row of
    windows, each a float32 sum below 4 moved by a few ulps of it (< 4 * 2^-22, about 1e-6), over at least 4096 windows (smaller
    pairs take the exact kernel, which shares no reciprocal): < 2 * 1e-6 / 4096 < 1e-9.  The pictures here are under 250 wide, so
    a row of windows is one block of columns."""
    images, rows = _images(), _rows(_odd_boxes_of)
    got, status = ctx.ssim_pairs_viewed(images, *_columns(rows))
    flat = [v for a, b, ba, bb, k in rows for v in (V.view(images[a], ba, 0), V.view(images[b], bb, k))]
    assert any(v.shape[0] * v.shape[1] % 4 for v in flat)
    want, want_status = ctx.ssim_pairs(flat, list(range(0, len(flat), 2)), list(range(1, len(flat), 2)))
    worst = 0.0
    for row, g, w, gs, ws in zip(rows, got.tolist(), want.tolist(), status.tolist(), want_status.tolist()):
        print(row, g, w, g - w)
        worst = max(worst, abs(g - w))
        assert gs == ws == 0 and abs(g - w) < 1e-9, row
    print("largest difference", worst)


def test_without_an_orientation_it_is_the_boxed_call_and_without_a_box_the_turned_one(ctx, pairs):
    images, rows = pairs["images"], pairs["rows"]
    a, b, box_a, box_b, orient = _columns(rows)
    want, want_status = ctx.ssim_pairs_boxed(images, a, b, box_a, box_b)
    for ob in (None, np.zeros(len(rows), np.int32)):
        got, status = ctx.ssim_pairs_viewed(images, a, b, box_a, box_b, ob)
        assert got.tolist() == want.tolist() and status.tolist() == want_status.tolist()
    want, want_status = ctx.ssim_pairs_turned(images, a, b, orient)
    assert not want_status.any()
    zeros = np.zeros((len(rows), 4), np.int32)
    size = lambda idx: np.array([(0, 0, images[i].shape[1], images[i].shape[0]) for i in idx], np.int32)
    for ba, bb in ((None, None), (zeros, zeros), (size(a), size(b)), (None, size(b)), (zeros, None)):
        got, status = ctx.ssim_pairs_viewed(images, a, b, ba, bb, orient)
        assert got.tolist() == want.tolist() and status.tolist() == want_status.tolist()


def test_the_four_pair_calls_share_one_scratch(ctx, pairs):
    """The made planes of every pair call lie in one scratch buffer of the context.  The turned, boxed, viewed and plain calls one
    after the other, then the other way round, then a smaller viewed batch twice behind the larger one: every answer is the first
    one of its kind, float64 == and the same statuses.  The smaller batch is every third row, and its answers are the larger one's
    for those rows too: all areas here are multiples of four (test_ssim_pairs_viewed_on_views_of_odd_areas says why that matters), so how a call stacks its planes does not show."""
    images, rows = pairs["images"], pairs["rows"]
    a, b, box_a, box_b, orient = _columns(rows)
    calls = {"turned": lambda: ctx.ssim_pairs_turned(images, a, b, orient), "boxed": lambda: ctx.ssim_pairs_boxed(images, a, b, box_a, box_b),
             "viewed": lambda: ctx.ssim_pairs_viewed(images, a, b, box_a, box_b, orient), "plain": lambda: ctx.ssim_pairs(images, a, b)}
    first = {}
    for name in list(calls) + list(calls)[::-1]:
        got, status = calls[name]()
        want = first.setdefault(name, (got.tolist(), status.tolist()))
        assert (got.tolist(), status.tolist()) == want, name
        assert not status.any() and np.isfinite(got).all(), name
    assert len({tuple(scores) for scores, _ in first.values()}) == 4                     # four different questions
    few = rows[::3]
    for _ in range(2):
        got, status = ctx.ssim_pairs_viewed(images, *_columns(few))
        assert got.tolist() == first["viewed"][0][::3] and status.tolist() == first["viewed"][1][::3]


def test_ssim_pairs_viewed_against_the_oracle(ctx, pairs):
    got, _ = ctx.ssim_pairs_viewed(pairs["images"], *_columns(pairs["rows"]))
    ctx.ssim_set_mode(True)
    try:
        exact, _ = ctx.ssim_pairs_viewed(pairs["images"], *_columns(pairs["rows"]))
    finally:
        ctx.ssim_set_mode(False)
    for row, g, e, w in zip(pairs["rows"], got.tolist(), exact.tolist(), pairs["oracle"]):
        print(row, g, e, w)
        assert abs(g - w) <= 1e-5, row
        assert abs(e - w) <= 1e-6, row


def test_statuses_a_box_outside_its_image_and_a_bad_orientation(ctx, pairs):
    images = pairs["images"][:2]                                                       # 96 x 80 and 80 x 96
    zero = (0, 0, 0, 0)
    # a box that leaves a common side under 7 -- for the last two only once b is turned; an index outside the images
    sc, st = ctx.ssim_pairs_viewed(images, [0, 0, 0, 1, 0, 0], [1, 1, 7, 0, 1, 1],
                                   [(5, 5, 11, 60), zero, zero, (0, 0, 80, 6), zero, zero],
                                   [zero, (0, 0, 80, 6), (9, 9, 9, 9), zero, (0, 0, 6, 96), (0, 0, 6, 96)], [0, 1, 4, 3, 5, 0])
    assert st.tolist() == [1, 1, 2, 1, 1, 1] and np.isnan(sc).all()
    sc, st = ctx.ssim_pairs_viewed(images, [0, 0], [1, 1], None, [(0, 0, 80, 7), (0, 0, 7, 96)], [4, 4])   # 7 x 80 and 96 x 7 once turned
    assert st.tolist() == [0, 0] and np.isfinite(sc).all()
    for bad in ((0, 0, 97, 80), (10, 0, 10, 80), (-1, 0, 50, 50), (0, 0, 96, 81), (0, 0, 0, 5)):
        with pytest.raises(ValueError, match="pair 1"):
            ctx.ssim_pairs_viewed(images, [0, 0], [1, 1], [zero, bad], [zero, zero], [0, 5])
    with pytest.raises(ValueError, match="pair 0"):
        ctx.ssim_pairs_viewed(images, [0], [1], None, [(0, 0, 81, 96)], [4])             # the box is of b as it lies, not as it is turned
    for bad in (8, -1):
        with pytest.raises(ValueError, match="pair 1"):
            ctx.ssim_pairs_viewed(images, [0, 0], [1, 1], None, None, [0, bad])


# ---- 3. the hashes ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pictures():
    """Bordered pictures of every kind, their originals, a uniform picture, a thin trim, a small box, in an order that mixes
    them: a ragged batch."""
    images = []
    for i, px in enumerate(T.originals()[:3]):
        images.append(px)
        for kind in T.BORDER_KINDS:
            images.append(T.bordered(px, kind)[0])
    images.append(np.full((64, 64, 3), 9, np.uint8))
    thin = np.full((100, 100, 3), 255, np.uint8)
    thin[1:, :] = T.originals()[3][:99, :100]
    images.append(thin)                                            # one row off 100: under 2 %
    small = np.full((60, 60, 3), 0, np.uint8)
    small[10:17, 10:40] = 255
    images.append(small)                                           # a side of 7
    return images


def _as_channels(px: np.ndarray, ch: int, i: int) -> np.ndarray:
    if ch == 1:
        return np.ascontiguousarray(px[:, :, 1])
    if ch == 4:
        return np.concatenate([px, np.full(px.shape[:2] + (1,), 7 * i, np.uint8)], axis=2)
    return px


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_hash_images_turned_trimmed_is_the_two_calls_and_the_oracles_turned_hashes_of_the_crop(ctx, pictures, ch):
    batch = [_as_channels(px, ch, i) for i, px in enumerate(pictures)]
    n = len(batch)
    t_want, t_status = ctx.hash_images_turned(batch)
    ph_want, box_want, has_want, c_status = ctx.hash_images_trimmed(batch, T.TOLERANCE)
    assert not t_status.any() and not c_status.any() and has_want.sum() >= 12 and (~has_want).sum() >= 3
    oracle = np.zeros((n, 8), np.uint64)
    for i, px in enumerate(batch):
        box, hashes = V.trimmed_turned_hashes(px)
        assert tuple(box_want[i].tolist()) == box and bool(has_want[i]) == (hashes is not None)
        if hashes is not None:
            oracle[i] = hashes
    # device pixels: every image at another address mod 16, with a gap before it
    gaps = [(5 * i + 1) % 16 for i in range(n)]
    offsets, at = [], 0
    for px, gap in zip(batch, gaps):
        at += gap
        offsets.append(at)
        at += px.size
    flat = np.full(at, 0x5A, np.uint8)
    for px, o in zip(batch, offsets):
        flat[o:o + px.size] = px.reshape(-1)
    dev = ctx.malloc(flat.nbytes)
    try:
        ctx.memcpy(dev, flat, flat.nbytes)
        on_device = ctx.hash_images_turned_trimmed_at(dev, offsets, [px.shape[1] for px in batch], [px.shape[0] for px in batch], ch, T.TOLERANCE)
    finally:
        ctx.free(dev)
    for where, (tn, cut, boxes, has, status) in (("host", ctx.hash_images_turned_trimmed(batch, T.TOLERANCE)), ("device", on_device)):
        assert not status.any(), where
        assert np.array_equal(tn, t_want), where
        assert np.array_equal(boxes, box_want) and np.array_equal(has, has_want) and np.array_equal(cut[:, 0], ph_want), where
        assert np.array_equal(cut, oracle), where
        assert not cut[~has].any() and cut[has].all(), where
    assert len({tuple(r) for r in oracle[has_want].tolist()}) >= 3 and all(len(set(r)) == 8 for r in oracle[has_want].tolist())


def test_hash_images_turned_trimmed_with_a_failed_image_and_nothing(ctx, pictures):
    n = 6
    batch = pictures[:n]
    offsets = np.cumsum([0] + [px.size for px in batch[:-1]]).astype(np.uint64)
    widths, heights = np.array([px.shape[1] for px in batch], np.int32), np.array([px.shape[0] for px in batch], np.int32)
    whole = ctx.hash_images_turned_trimmed(batch, T.TOLERANCE)
    widths[3] = 0                                                                   # a failed image in the middle
    flat = np.concatenate([px.reshape(-1) for px in batch])
    tn, cut, boxes, has, status = ctx.hash_images_turned_trimmed_at(flat, offsets, widths, heights, 3, T.TOLERANCE)
    assert status.tolist() == [0, 0, 0, 1, 0, 0]
    assert not tn[3].any() and not cut[3].any() and not boxes[3].any() and not has[3]
    keep = [0, 1, 2, 4, 5]
    for got, want in zip((tn, cut, boxes, has), whole[:4]):
        assert np.array_equal(got[keep], want[keep])
    assert [a.shape for a in ctx.hash_images_turned_trimmed([], 48)] == [(0, 8), (0, 8), (0, 4), (0,), (0,)]
    with pytest.raises(ValueError):
        ctx.hash_images_turned_trimmed(batch, 256)


# ---- 4. the seam ---------------------------------------------------------------------------------------------------------------------
# (border kind or None, the orientation the bordered picture is turned by): a box turned, a box as it lies, a whole picture turned
SEAM_CASES = (("letterbox", 5), ("white margins", 2), ("pillarbox", 6), ("grey frame", 0), (None, 3))


@pytest.mark.parametrize("ext", ["png", "jpg"])
def test_refine_turned_trimmed_pairs_at_the_seam(ctx, tmp_path, ext):
    from PIL import Image

    px = T.originals()[1]
    how = {"quality": 95} if ext == "jpg" else {}
    path_a = str(tmp_path / f"a.{ext}")
    Image.fromarray(px).save(path_a, **how)
    with Image.open(path_a) as opened:
        a = opened.convert("RGB")
        a.load()
    rows, view_rows, off_rows, whole_rows, loader_rows, swapped, swapped_views = [], [], [], [], [], [], []
    for n, (kind, k) in enumerate(SEAM_CASES):
        back = turned.INVERSE[k]
        path_b = str(tmp_path / f"b{n}.{ext}")
        Image.fromarray(TC.turn_k(k, px if kind is None else T.bordered(px, kind)[0])).save(path_b, **how)
        with Image.open(path_b) as opened:
            b = opened.convert("RGB")
            b.load()
        box = T.content_box(np.asarray(b), T.TOLERANCE) if kind else None
        assert box is None or T.qualifies(b.width, b.height, box)
        # the files refine_pairs sees: Pillow's crop(box).transpose(...) of what Pillow reads from b_n, stored without loss
        path_c = str(tmp_path / f"c{n}.png")
        V.pillow_view(b, box, back).save(path_c)
        path_ppm = str(tmp_path / f"b{n}.ppm")              # no GPU decoder takes a PPM file: the loader's route
        b.save(path_ppm)
        rows.append((1, 10 + n, path_a, path_b, False, kind is not None, back))
        view_rows.append((1, 10 + n, path_a, path_c))
        off_rows.append((1, 10 + n, path_a, path_b, False, False, 0))
        whole_rows.append((1, 10 + n, path_a, path_b))
        loader_rows.append((1, 10 + n, path_a, path_ppm, False, kind is not None, back))
        # the bordered file first: its box as it lies against the original turned its way
        path_d, path_e = str(tmp_path / f"d{n}.png"), str(tmp_path / f"e{n}.png")
        V.pillow_view(b, box, 0).save(path_d)
        V.pillow_view(a, None, k).save(path_e)
        swapped.append((10 + n, 1, path_b, path_a, kind is not None, False, k))
        swapped_views.append((10 + n, 1, path_d, path_e))
    cfg = refine.RefinementThresholds(ssim=0.9)
    stats: dict = {}
    got = refine.refine_turned_trimmed_pairs(rows, thresholds=cfg, stats=stats)
    want = refine.refine_pairs(view_rows, thresholds=cfg)
    assert (stats["pairs"], stats["decodes"], stats["box_files"]) == (5, 6, 4)
    assert (stats["crop_launches"], stats["turn_launches"], stats["view_launches"]) == (1, 1, 1)
    for n, (g, w) in enumerate(zip(got, want)):
        print(ext, SEAM_CASES[n], g.ssim, w.ssim)
        assert g == w and g.is_duplicate and (g.file_id_a, g.file_id_b) == (1, 10 + n), n     # dataclass equality: the float compared with ==
    assert refine.refine_turned_trimmed_pairs(swapped, thresholds=cfg) == refine.refine_pairs(swapped_views, thresholds=cfg)
    # the flags off and no orientation: the whole files, as refine_pairs scores them -- and then nothing of it is a copy
    off_stats: dict = {}
    off = refine.refine_turned_trimmed_pairs(off_rows, thresholds=cfg, stats=off_stats)
    assert off == refine.refine_pairs(whole_rows, thresholds=cfg)
    assert (off_stats["box_files"], off_stats["crop_launches"], off_stats["turn_launches"], off_stats["view_launches"]) == (0, 0, 0, 0)
    assert not any(r.is_duplicate for r, (kind, k) in zip(off, SEAM_CASES) if k)
    by_loader: dict = {}
    assert refine.refine_turned_trimmed_pairs(loader_rows, thresholds=cfg, stats=by_loader) == got
    assert by_loader["decodes"] == 6 and by_loader["gpu_decodes"] <= 1          # at most a itself was decoded on the device
    # an unreadable file gives None, in place
    missing = refine.refine_turned_trimmed_pairs([rows[1], (1, 99, path_a, str(tmp_path / "absent.png"), False, True, 5), rows[3]], thresholds=cfg)
    assert missing[1] is None and missing[0] == got[1] and missing[2] == got[3]
    # a flagged side whose picture has no box at the seam is scored as it lies, turned
    path_flat, path_flat_turned = str(tmp_path / "flat.png"), str(tmp_path / "flat_turned.png")
    Image.fromarray(np.full((96, 128, 3), 90, np.uint8)).save(path_flat)
    Image.fromarray(np.full((128, 96, 3), 90, np.uint8)).save(path_flat_turned)
    assert refine.refine_turned_trimmed_pairs([(1, 50, path_a, path_flat, False, True, 5)], thresholds=cfg) == \
        refine.refine_pairs([(1, 50, path_a, path_flat_turned)], thresholds=cfg)
    with pytest.raises(ValueError):
        refine.refine_turned_trimmed_pairs(rows, tolerance=256)
    with pytest.raises(ValueError):
        refine.refine_turned_trimmed_pairs([rows[0][:6] + (8,)])


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from PIL import Image

    folder = tmp_path_factory.mktemp("turned_trimmed_files")
    records = V.write_corpus(folder)
    opened = [np.asarray(Image.open(r["path"]).convert("RGB")) for r in records]
    assert max(max(px.shape[:2]) for px in opened) <= 260
    stored, _, ok = K.hash_batch(opened, want_dhash=False)
    assert ok.all()
    files = [DuplicateFile(r["file_id"], Path(r["path"]), os.path.getsize(r["path"]), px.shape[1], px.shape[0], int(h))
             for r, px, h in zip(records, opened, stored)]
    return dict(folder=folder, records=records, opened=opened, files=files)


def _groups(clusters):
    return {frozenset(e.file.file_id for e in c.files) for c in clusters}


def test_without_a_threshold_every_planted_copy_and_every_decoy_is_linked_and_the_two_modes_are_covered(corpus):
    records, files = corpus["records"], corpus["files"]
    original = V.original_of(records)
    clusters, matches = api.find_turned_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD)
    assert all(m.ssim is None and m.file_id_a < m.file_id_b for m in matches)
    found = {(m.file_id_a, m.file_id_b): m for m in matches}
    assert len(found) == len(matches)
    for r in records:
        if r["planted"] or r["decoy"]:
            m = found[(original[r["family"]], r["file_id"])]
            print(r["path"], m)
            assert (m.trimmed_a, m.trimmed_b, m.orientation) == (False, True, turned.INVERSE[r["orientation"]]), r
            assert m.box_a is None and m.box_b == T.content_box(corpus["opened"][r["file_id"] - 1], T.TOLERANCE), r
            assert any({m.file_id_a, m.file_id_b} <= g for g in _groups(clusters))
    # what the two existing modes find on the same files, the new call finds too, at no larger a distance
    _, turned_matches = api.find_turned_duplicates(files, hamming_threshold=T.THRESHOLD)
    _, trimmed_matches = api.find_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD)
    assert len(turned_matches) >= 2 * len(TC.PLANTED) and len(trimmed_matches) >= 16
    for m in turned_matches + trimmed_matches:
        assert found[(m.file_id_a, m.file_id_b)].hamming <= m.hamming, m
    # and neither of them links a planted copy to its original
    old_pairs = {(m.file_id_a, m.file_id_b) for m in turned_matches + trimmed_matches}
    assert not any((original[r["family"]], r["file_id"]) in old_pairs for r in records if r["planted"])


def test_with_the_threshold_the_groups_are_the_families_and_scan_dups_prints_them(corpus, tmp_path, capsys):
    records, files, opened = corpus["records"], corpus["files"], corpus["opened"]
    decoys = {r["file_id"] for r in records if r["decoy"]}
    families, original = V.families(records), V.original_of(records)
    clusters, matches = api.find_turned_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD, ssim_threshold=V.SSIM_THRESHOLD)
    assert _groups(clusters) == families
    found = {(m.file_id_a, m.file_id_b): m for m in matches}
    assert not any({a, b} & decoys for a, b in found)
    for r in records:
        if r["planted"]:
            assert found[(original[r["family"]], r["file_id"])].orientation == turned.INVERSE[r["orientation"]], r
    for m in matches:
        box = lambda f, cut: T.content_box(opened[f - 1], T.TOLERANCE) if cut else None
        want = O.ssim_fit(V.view(opened[m.file_id_a - 1], box(m.file_id_a, m.trimmed_a), 0),
                          V.view(opened[m.file_id_b - 1], box(m.file_id_b, m.trimmed_b), m.orientation))
        print(m, want)
        assert m.ssim >= V.SSIM_THRESHOLD and abs(m.ssim - want) <= 1e-5, m
    # the command line: the same groups, an orientation and a box column
    db = str(tmp_path / "k.db")
    conn = sqlite3.connect(db)
    conn.execute("CREATE TABLE files (id INTEGER PRIMARY KEY, path TEXT, size INTEGER, width INTEGER, height INTEGER, is_present INTEGER)")
    conn.execute("CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER, dhash_u64 INTEGER)")
    for f in files:
        conn.execute("INSERT INTO files VALUES (?, ?, ?, ?, ?, 1)", (f.file_id, str(f.path), f.size, f.width, f.height))
        conn.execute("INSERT INTO signatures VALUES (?, ?, 0)", (f.file_id, O.to_signed64(f.phash)))
    conn.commit()
    conn.close()
    out_csv = str(tmp_path / "out.csv")
    assert cli.main(["scan-dups", "--db", db, "--turned-trimmed", "--turned-trimmed-ssim", str(V.SSIM_THRESHOLD), "--csv", out_csv]) == 0
    assert f"{len(families)} duplicate group(s), {sum(map(len, families))} file(s)" in capsys.readouterr().out
    with open(out_csv, newline="") as handle:
        table = list(csv.DictReader(handle))
    assert list(table[0]) == cli.CSV_HEADER + ["orientation", "box"]
    groups: dict = {}
    for row in table:
        groups.setdefault(row["group"], set()).add(int(row["file_id"]))
    assert {frozenset(g) for g in groups.values()} == families
    by_id = {int(row["file_id"]): row for row in table}
    for r in records:
        if r["planted"]:
            assert by_id[r["file_id"]]["box"] == " ".join(str(v) for v in T.content_box(opened[r["file_id"] - 1], T.TOLERANCE)), r
            assert by_id[r["file_id"]]["orientation"] != "" or by_id[r["file_id"]]["keeper"] == "1", r
