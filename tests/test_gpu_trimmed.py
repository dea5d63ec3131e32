"""Bordered copies on the GPU: ke_content_boxes and ke_crop_pack (csrc/ke_trim.hip), ke_hash_images_trimmed, and what is
built on them.

The boxes are integers and are held to the definition (tests/_trim_cases.py content_box, which tests/test_trim_core_cpu.py
holds to the Pillow recipe on the same grid); the crops are bytes; the hashes are held bit for bit to ``ctx.hash_images`` of
the crops and to the oracle's ``O.hash_image`` of the crops.  That the crop's hash stands for the original's, JPEG loss
included, is tests/test_trimmed_cpu.py's business (at most 3 bits on these very pictures)."""
from __future__ import annotations

import csv
import os
import sqlite3
from pathlib import Path

import numpy as np
import pytest

import _trim_cases as T
import kobato_eyes_amd as K
from kobato_eyes_amd import _native, api, cli, trimmed
from kobato_eyes_amd.scanner import DuplicateFile, DuplicateScanConfig, DuplicateScanner, TrimmedMatch
from oracle import oracle as O

pytestmark = pytest.mark.gpu
BAND = 32          # KE_TRIM_BAND_ROWS (tests/test_trim_core_cpu.py checks the header says so)


@pytest.fixture(scope="module")
def ctx():
    return _native.get_context(0)


class _Device:
    """Host bytes in a device buffer of the context, freed on exit."""

    def __init__(self, ctx, host: np.ndarray):
        self.ctx, self.host = ctx, host
        self.ptr = ctx.malloc(max(host.nbytes, 16))

    def __enter__(self):
        self.ctx.memcpy(self.ptr, self.host, self.host.nbytes)
        return self.ptr

    def __exit__(self, *exc):
        self.ctx.free(self.ptr)

    def read(self) -> np.ndarray:
        out = np.empty_like(self.host)
        self.ctx.memcpy(out, self.ptr, out.nbytes)
        return out


def _pack_at(images, alignments) -> tuple:
    """The images in one buffer, image i starting ``alignments[i]`` bytes past a multiple of 16 with a gap in front."""
    offsets, at = [], 0
    for px, a in zip(images, alignments):
        at = (at + 16 + 15) // 16 * 16 + a
        offsets.append(at)
        at += px.size
    flat = np.full(at + 16, 0x5A, np.uint8)
    for px, off in zip(images, offsets):
        flat[off:off + px.size] = px.reshape(-1)
    return flat, np.array(offsets, np.uint64)


def _seam_images(ch: int) -> tuple:
    """(images, boxes): a 1024 x 512 and a 64 x 3000 image, each with a single differing pixel on a band seam (the last row of
    one band, the first of the next), in the last row and in the last column."""
    images, boxes = [], []
    for w, h in ((1024, 512), (64, 3000)):
        for x, y in ((w // 3, 5 * BAND - 1), (w // 3 + 1, 5 * BAND), (7, h - 1), (w - 1, h // 2 + 1)):
            px = np.full((h, w, ch), 200, np.uint8)
            px[y, x, 0] = 100
            images.append(px[:, :, 0] if ch == 1 else px)
            boxes.append((x, y, x + 1, y + 1))
    return images, boxes


@pytest.fixture(scope="module")
def grid():
    """{channels: (images, alignments)}: the CPU grid's pictures, each at every alignment 0..15, then the seam images."""
    rng = np.random.default_rng(T.SEED)
    out = {}
    for ch in (1, 3, 4):
        images, aligns = [], []
        for w, h in T.grid_shapes(BAND):
            px = T.grid_picture(rng, w, h, ch)
            for a in range(16):
                images.append(px)
                aligns.append(a)
        seams, _ = _seam_images(ch)
        images += seams
        aligns += [(3 * i + 1) % 16 for i in range(len(seams))]
        out[ch] = (images, aligns)
    return out


# ---- ke_content_boxes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_content_boxes_equal_the_definition_on_the_whole_grid_at_every_alignment(ctx, grid, ch):
    images, aligns = grid[ch]
    assert len(images) == 12 * 13 * 16 + 8
    flat, offsets = _pack_at(images, aligns)
    widths, heights = [px.shape[1] for px in images], [px.shape[0] for px in images]
    distinct = {id(px): px for px in images}
    with _Device(ctx, flat) as dev:
        assert sorted({int((dev + int(o)) % 16) for o in offsets}) == list(range(16))
        for tol in T.TOLERANCES:
            want_of = {k: T.content_box(px, tol) for k, px in distinct.items()}
            want = np.array([want_of[id(px)] for px in images], np.int32)
            boxes, status = ctx.content_boxes_at(dev, offsets, widths, heights, ch, tol)
            assert not status.any()
            wrong = np.nonzero((boxes != want).any(axis=1))[0]
            assert len(wrong) == 0, (tol, [(widths[i], heights[i], aligns[i], boxes[i].tolist(), want[i].tolist()) for i in wrong[:5]])
            if tol == 255:
                assert not boxes.any()
    # the seam images hold what they were made to hold
    _, seam_boxes = _seam_images(ch)
    assert [tuple(b) for b in want[-8:].tolist()] == [(0, 0, 0, 0)] * 8                  # at 255
    got, _ = ctx.content_boxes(images[-8:], 48)
    assert [tuple(b) for b in got.tolist()] == seam_boxes


def _long_row_images(tol: int) -> list:
    """701 x 5 RGB pictures whose corner colour differs from channel to channel, for the rows of over 1024 bytes, where a lane
    of the box kernel takes a second and a third vector and turns its three patterns round: one picture with every byte within
    ``tol`` of its own channel's reference (random, the extremes among them), then pictures with a single byte at
    ref[c] +- tol and at ref[c] +- (tol + 1), for every channel, in a lane's second vector and in its third."""
    w, h, ref = 701, 5, np.array([10, 120, 240], np.int64)
    rng = np.random.default_rng(T.SEED + tol)
    base = np.empty((h, w, 3), np.uint8)
    base[:] = ref
    within = np.clip(ref + rng.integers(-tol, tol + 1, size=(h, w, 3)), 0, 255).astype(np.uint8)
    within[:, ::2] = np.clip(ref + rng.choice([-tol, tol], size=(h, (w + 1) // 2, 3)), 0, 255)
    within[0, 0] = ref
    images = [within]
    for x, y in ((400, 1), (690, 3)):                       # bytes 1200.. and 2070.. of the row
        assert 1024 <= 3 * x < 2048 or 3 * x >= 2048
        for c in range(3):
            for d in (tol, -tol, tol + 1, -tol - 1):
                if 0 <= ref[c] + d <= 255:
                    px = base.copy()
                    px[y, x, c] = ref[c] + d
                    images.append(px)
    return images


@pytest.mark.parametrize("tol", [0, 1, 15, 48])
def test_content_boxes_of_rows_over_1024_bytes_keep_each_channel_to_its_own_reference(ctx, tol):
    """The pattern a lane holds for a dword depends on the channel of the dword's first byte, and for 3 channels it moves on by
    one with every 64 vectors: a wrong turn compares a byte with another channel's reference, which shows only where the
    three references differ by more than the tolerance (10, 120, 240)."""
    pictures = _long_row_images(tol)
    images = [px for px in pictures for _ in range(16)]
    aligns = [a for _ in pictures for a in range(16)]
    want = np.array([T.content_box(px, tol) for px in images], np.int32)
    # the pictures hold what they were made to hold: no box within the tolerance, one pixel beyond it, in all three channels
    assert not want[:16].any() and want[16:].any(axis=1).sum() >= 16 * 8 and (~want[16:].any(axis=1)).sum() >= 16 * 8
    assert {tuple(b) for b in want[want.any(axis=1)].tolist()} == {(400, 1, 401, 2), (690, 3, 691, 4)}
    flat, offsets = _pack_at(images, aligns)
    with _Device(ctx, flat) as dev:
        boxes, status = ctx.content_boxes_at(dev, offsets, [701] * len(images), [5] * len(images), 3, tol)
    assert not status.any()
    wrong = np.nonzero((boxes != want).any(axis=1))[0]
    assert len(wrong) == 0, (tol, [(int(i) // 16, aligns[i], boxes[i].tolist(), want[i].tolist()) for i in wrong[:5]])


def test_content_boxes_of_host_pixels_single_pixels_uniform_images_and_nothing(ctx):
    for ch in (1, 3, 4):
        for tol in T.TOLERANCES:
            cases = T.single_pixel_cases(ch, tol)
            got, status = ctx.content_boxes([px for _, px, _ in cases], tol)
            assert not status.any()
            assert [tuple(b) for b in got.tolist()] == [want for _, _, want in cases], (ch, tol)
        flatpx = np.full((70, 37, ch), 77, np.uint8)
        got, _ = ctx.content_boxes([flatpx[:, :, 0] if ch == 1 else flatpx], 0)
        assert got.tolist() == [[0, 0, 0, 0]]
    boxes, status = ctx.content_boxes([], 48)
    assert boxes.shape == (0, 4) and status.shape == (0,)
    boxes, status = ctx.content_boxes_at(np.zeros(16, np.uint8), np.zeros(0, np.uint64), [], [], 3, 48)
    assert boxes.shape == (0, 4)
    # an image without pixels has a status and four zeros; its neighbour is not disturbed
    px = np.zeros((9, 9, 3), np.uint8)
    px[4, 5] = 255
    flat = np.concatenate([px.reshape(-1), px.reshape(-1)])
    boxes, status = ctx.content_boxes_at(flat, [0, 243], [9, 0], [9, 9], 3, 48)
    assert status.tolist() == [0, 1] and boxes.tolist() == [[5, 4, 6, 5], [0, 0, 0, 0]]


# ---- ke_crop_pack ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3, 4])
def test_crop_pack_copies_the_box_at_every_alignment_and_writes_nothing_else(ctx, ch):
    rng = np.random.default_rng(T.SEED + ch)
    images, src_align, boxes, dst_align = [], [], [], []
    for sa in range(4):
        for da in range(4):
            for (w, h), (x0, y0, bw, bh) in (((37, 9), (sa + 1, 2, 21, 5)), ((300, 41), (da + 3, 0, 290 - sa, 41)), ((5, 6), (0, 0, 5, 6)),
                                             ((9, 7), (8, 6, 1, 1)), ((131, 70), (1, 3, 2 + da, 66))):
                images.append(rng.integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8))
                src_align.append(sa)
                boxes.append((x0, y0, x0 + bw, y0 + bh))
                dst_align.append(da)
    flat, src_off = _pack_at(images, src_align)
    crops = [T.crop(px, b) for px, b in zip(images, boxes)]
    dst_flat, dst_off = _pack_at(crops, dst_align)                  # the expected destination: 0x5A guards round every plane
    dst_start = np.full_like(dst_flat, 0x5A)
    src, dst = _Device(ctx, flat), _Device(ctx, dst_start)
    with src as s, dst as d:
        assert sorted({int((s + int(o)) % 4) for o in src_off}) == [0, 1, 2, 3] == sorted({int((d + int(o)) % 4) for o in dst_off})
        ctx.crop_pack(s, src_off, [px.shape[1] for px in images], [px.shape[0] for px in images], ch, boxes, d, dst_off)
        got = dst.read()
    assert np.array_equal(got, dst_flat)
    for bad in ((0, 0, 0, 5), (0, 0, 38, 5), (-1, 0, 5, 5), (3, 4, 3, 6)):
        with pytest.raises(ValueError):
            with _Device(ctx, flat) as s, _Device(ctx, dst_start) as d:
                ctx.crop_pack(s, src_off[:1], [37], [9], ch, [bad], d, dst_off[:1])


# ---- ke_hash_images_trimmed -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pictures():
    """Bordered pictures of every kind, their originals, a uniform picture, thin trims, a small box: (images, boxes by the
    definition, the oracle's hash of every qualifying crop or None), in an order that mixes them."""
    images = []
    for i, px in enumerate(T.originals()[:3]):
        images.append(px)
        for kind in T.BORDER_KINDS:
            images.append(T.bordered(px, kind)[0])
    images.append(np.full((64, 64, 3), 9, np.uint8))
    thin = np.full((100, 100, 3), 255, np.uint8)
    thin[1:, :] = T.originals()[3][:99, :100]
    images.append(thin)                                            # one row off 100: under 2 %
    two = np.full((100, 100, 3), 255, np.uint8)
    two[2:, :] = T.originals()[3][:98, :100]
    images.append(two)                                             # two rows off 100: qualifies
    small = np.full((60, 60, 3), 0, np.uint8)
    small[10:17, 10:40] = 255
    images.append(small)                                           # a side of 7
    boxes = [T.content_box(px, T.TOLERANCE) for px in images]
    want = [O.hash_image(T.crop(px, b))[0] if T.qualifies(px.shape[1], px.shape[0], b) else None for px, b in zip(images, boxes)]
    return images, boxes, want


def test_hash_images_trimmed_equals_the_hashes_of_the_crops(ctx, pictures):
    images, boxes, want = pictures
    assert sum(w is not None for w in want) >= 13 and sum(w is None for w in want) >= 3
    ph, got_boxes, has, status = ctx.hash_images_trimmed(images, T.TOLERANCE)
    assert not status.any()
    assert [tuple(b) for b in got_boxes.tolist()] == boxes
    assert has.tolist() == [w is not None for w in want]
    assert ph.tolist() == [w or 0 for w in want]                                  # the oracle's, in input order; 0 without a box
    crops = [T.crop(px, b) for px, b, w in zip(images, boxes, want) if w is not None]
    plain, _, st = ctx.hash_images(crops, want_dhash=False)
    assert not st.any() and plain.tolist() == ph[has].tolist()
    # the lossless bordered pictures hash as their originals
    for i in range(3):
        assert ph[5 * i + 1: 5 * i + 5].tolist() == [O.hash_image(images[5 * i])[0]] * 4


def test_hash_images_trimmed_on_device_pixels_other_channels_and_a_failed_image(ctx, pictures):
    images, boxes, want = pictures
    flat, offsets = _pack_at(images, [(5 * i + 1) % 16 for i in range(len(images))])
    n = len(images)
    widths, heights = np.array([px.shape[1] for px in images], np.int32), np.array([px.shape[0] for px in images], np.int32)
    widths[3] = 0                                                                   # a failed image in the middle
    ph, bx, has, status = np.zeros(n, np.uint64), np.zeros((n, 4), np.int32), np.zeros(n, np.uint8), np.zeros(n, np.int32)
    with _Device(ctx, flat) as dev:
        rc = ctx._lib.ke_hash_images_trimmed(ctx._h, dev, offsets.ctypes.data, widths.ctypes.data, heights.ctypes.data, 3, n, T.TOLERANCE,
                                             ph.ctypes.data, bx.ctypes.data, has.ctypes.data, status.ctypes.data)
    assert rc == 0
    assert status.tolist() == [0, 0, 0, 1] + [0] * (n - 4)
    assert ph[3] == 0 and has[3] == 0 and not bx[3].any()
    keep = [i for i in range(n) if i != 3]
    assert ph[keep].tolist() == [want[i] or 0 for i in keep] and [tuple(b) for b in bx[keep].tolist()] == [boxes[i] for i in keep]
    # one and four channels: the same picture's luma / the picture with a fourth byte
    grey = [np.ascontiguousarray(px[:, :, 1]) for px in images[:10]]
    rgba = [np.concatenate([px, np.full(px.shape[:2] + (1,), 7 * i, np.uint8)], axis=2) for i, px in enumerate(images[:10])]
    for batch in (grey, rgba):
        ph, bx, has, status = ctx.hash_images_trimmed(batch, T.TOLERANCE)
        for px, h, b, t in zip(batch, ph.tolist(), bx.tolist(), has.tolist()):
            box = T.content_box(px, T.TOLERANCE)
            assert tuple(b) == box
            assert t == T.qualifies(px.shape[1], px.shape[0], box)
            assert h == (O.hash_image(T.crop(px, box))[0] if t else 0)
    assert ctx.hash_images_trimmed([], 48)[0].shape == (0,)


# ---- trimmed_edges -----------------------------------------------------------------------------------------------------------
def test_trimmed_edges_equals_the_oracle_construction(monkeypatch):
    monkeypatch.delenv("KE_DUP_BUCKET_PAIR_CAP", raising=False)
    rng = np.random.default_rng(T.SEED + 9)
    n = 300
    stored = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    cut = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    has = rng.integers(0, 4, size=n) != 0
    flip = lambda v, k: np.uint64(int(v) ^ int(sum(1 << int(b) for b in rng.choice(64, size=k, replace=False))))
    for i in range(0, 120, 3):                    # trimmed i+1 looks like stored i; trimmed i+2 like trimmed i+1
        has[i + 1] = has[i + 2] = True
        cut[i + 1] = flip(stored[i], i % 10)
        cut[i + 2] = flip(cut[i + 1], (i // 3) % 10)
    cut[200] = stored[200]                        # a file against its own crop
    files = [DuplicateFile(1000 + i, Path(f"lib/{i}.png"), 1000 + 37 * (i % 50), 100, 100, int(stored[i])) for i in range(n)]
    boxes = rng.integers(0, 90, size=(n, 4)).astype(np.int32)
    for ratio in (None, 0.7):
        cfg = DuplicateScanConfig(hamming_threshold=T.THRESHOLD, size_ratio=ratio)
        got = DuplicateScanner(cfg).trimmed_edges(files, cut, has, boxes)
        with monkeypatch.context() as m:
            stand_in = T.OracleScanContext()
            m.setattr(_native, "get_context", lambda device=0, role="": stand_in)
            want = DuplicateScanner(cfg).trimmed_edges(files, cut, has, boxes)
        assert got == want and len(want) >= (60 if ratio is None else 20)
        assert all(isinstance(mt, TrimmedMatch) and mt.file_id_a < mt.file_id_b for mt in got)
        assert any(mt.trimmed_a and mt.trimmed_b for mt in got) and any(not mt.trimmed_a for mt in got)


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The files on disk, their DuplicateFile rows with the stored pHash (the pixels Pillow opens, hashed here), and the
    result of find_trimmed_duplicates: made once."""
    from PIL import Image

    folder = tmp_path_factory.mktemp("trimmed_files")
    records = T.write_files(folder)
    assert len(records) == 4 + 16 + 2
    opened = [np.asarray(Image.open(r["path"]).convert("RGB")) for r in records]
    assert max(max(px.shape[:2]) for px in opened) <= 256
    stored, _, ok = K.hash_batch(opened, want_dhash=False)
    assert ok.all()
    files = [DuplicateFile(r["file_id"], Path(r["path"]), os.path.getsize(r["path"]), px.shape[1], px.shape[0], int(h))
             for r, px, h in zip(records, opened, stored)]
    clusters, matches = api.find_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD)
    return dict(folder=folder, records=records, opened=opened, files=files, clusters=clusters, matches=matches)


def _wanted_groups(records) -> set:
    groups: dict = {}
    for r in records:
        groups.setdefault(r["original"], set()).add(r["file_id"])
    return {frozenset(v) for v in groups.values()}


def test_the_stored_hashes_alone_link_none_of_them(library):
    """The test that shows the feature: find_duplicates on the same rows finds nothing."""
    assert api.find_duplicates(library["files"], hamming_threshold=T.THRESHOLD) == []


def test_find_trimmed_duplicates_links_every_copy_to_its_original_and_the_two_canvases(library):
    records, matches = library["records"], library["matches"]
    got = {(m.file_id_a, m.file_id_b): m for m in matches}
    original = {r["original"]: r["file_id"] for r in records if r["kind"] is None}
    for r in records:
        if r["kind"] is None or r["original"] == "drawing":
            continue
        m = got[(original[r["original"]], r["file_id"])]              # the copy against its original as it is
        assert (m.trimmed_a, m.trimmed_b) == (False, True) and m.hamming <= T.THRESHOLD and m.box_a is None
        px = library["opened"][r["file_id"] - 1]
        assert m.box_b == T.content_box(px, T.TOLERANCE)
    a, b = (r["file_id"] for r in records if r["original"] == "drawing")
    m = got[(a, b)]
    assert (m.trimmed_a, m.trimmed_b, m.hamming) == (True, True, 0) and m.box_a == (60, 20, 210, 130) and m.box_b == (11, 97, 161, 207)
    assert {frozenset(e.file.file_id for e in c.files) for c in library["clusters"]} == _wanted_groups(records)


def test_trimmed_signatures_are_the_oracles_on_the_files_pixels(library):
    paths = [r["path"] for r in library["records"]] + [str(library["folder"] / "missing.png")]
    hashes, boxes, has, ok = trimmed.trimmed_signatures(paths)
    n = len(library["records"])
    assert ok.tolist() == [True] * n + [False] and hashes[-1] == 0 and not has[-1] and not boxes[-1].any()
    for h, b, t, px in zip(hashes.tolist(), boxes.tolist(), has.tolist(), library["opened"]):
        box = T.content_box(px, T.TOLERANCE)
        assert tuple(b) == box and t == T.qualifies(px.shape[1], px.shape[0], box)
        assert h == (O.hash_image(T.crop(px, box))[0] if t else 0)


def test_scan_dups_trimmed_writes_the_same_groups_with_the_box_column(library, tmp_path, capsys):
    files = library["files"]
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
    assert cli.main(["scan-dups", "--db", db, "--trimmed", "--csv", out_csv]) == 0
    assert "5 duplicate group(s), 22 file(s)" in capsys.readouterr().out
    with open(out_csv, newline="") as handle:
        rows = list(csv.DictReader(handle))
    assert list(rows[0]) == cli.CSV_HEADER + ["box"]
    groups: dict = {}
    for r in rows:
        groups.setdefault(r["group"], set()).add(int(r["file_id"]))
    assert {frozenset(g) for g in groups.values()} == {frozenset(e.file.file_id for e in c.files) for c in library["clusters"]}
    kind = {r["file_id"]: r["kind"] for r in library["records"]}
    for r in rows:
        px = library["opened"][int(r["file_id"]) - 1]
        want = "" if kind[int(r["file_id"])] is None else " ".join(str(v) for v in T.content_box(px, T.TOLERANCE))
        assert r["box"] == want, r["path"]
    # a tolerance under which the JPEG copies' borders no longer read as border changes the result, so the flag arrives
    assert cli.main(["scan-dups", "--db", db, "--trimmed", "--trim-tolerance", "255", "--csv", out_csv]) == 0
    assert "0 duplicate group(s), 0 file(s)" in capsys.readouterr().out
    # without the flag the command does what it did: no box column, nothing linked
    assert cli.main(["scan-dups", "--db", db, "--csv", out_csv]) == 0
    with open(out_csv, newline="") as handle:
        assert handle.read().strip() == ",".join(cli.CSV_HEADER)
    for other in (["--turned"], ["--added-like", "%x%"], ["--refine"]):
        with pytest.raises(ValueError, match="--trimmed cannot be combined"):
            cli.main(["scan-dups", "--db", db, "--trimmed", *other])
