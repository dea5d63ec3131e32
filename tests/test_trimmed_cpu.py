"""Trimmed pHashes and the table of DuplicateScanner.trimmed_edges without a GPU.

* The precondition of tests/test_gpu_trimmed.py, on the CPU oracle alone.  On the case builder's lossless pictures (six
  originals of 97 x 64 to 256 x 144 under the issue's four border kinds) the Pillow recipe yields the placed rectangle and
  the oracle's pHash of the Pillow crop equals the oracle's pHash of the original bit for bit, while the bordered picture's
  own pHash lies more than the threshold from it.  On their JPEG copies (quality 85) at tolerance 48 the box is at most one
  pixel too large on any side and the crop's pHash lies within the scan's threshold of 8 of the original's: the largest
  distance found on these 24 copies is 3 bits (a grey frame round the 160 x 120 and the 200 x 150 picture).
* DuplicateScanner.trimmed_edges and api.find_trimmed_duplicates against a stand-in context whose hamming_scan is the
  oracle's banded scan filtered by b >= first_new -- what ke_hamming_scan_from is specified to return: the table (hashes,
  ids, sizes, first_new) and the reduction to one match per pair.
* scan-dups refuses --trimmed together with --turned, --added-like or --refine."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import _trim_cases as T
from kobato_eyes_amd import _native, api, cli, trimmed
from kobato_eyes_amd.scanner import DuplicateFile, DuplicateScanConfig, DuplicateScanner, TrimmedMatch
from oracle import oracle as O

MASK = (1 << 64) - 1
JPEG_WORST = 3          # the largest distance this file found; the assertion below is the scan's threshold


# ---- the precondition of the GPU tests ------------------------------------------------------------------------------------
def test_lossless_crops_hash_as_their_originals_and_jpeg_copies_stay_within_the_threshold():
    worst = 0
    for i, px in enumerate(T.originals()):
        own = O.hash_image(px)[0]
        for kind in T.BORDER_KINDS:
            pic, placed = T.bordered(px, kind)
            h, w = pic.shape[:2]
            assert T.pillow_box(pic, T.TOLERANCE) == placed == T.content_box(pic, T.TOLERANCE), (i, kind)
            assert T.qualifies(w, h, placed), (i, kind)
            assert O.hash_image(T.crop(pic, placed))[0] == own, (i, kind)
            assert O.hamming64(O.hash_image(pic)[0], own) > T.THRESHOLD, (i, kind)           # the pHash does not survive the border
            lossy = T.through_jpeg(pic)
            box = T.pillow_box(lossy, T.TOLERANCE)
            assert box == T.content_box(lossy, T.TOLERANCE)
            assert all(0 <= placed[k] - box[k] <= 1 for k in (0, 1)) and all(0 <= box[k] - placed[k] <= 1 for k in (2, 3)), (i, kind, box, placed)
            assert T.qualifies(w, h, box), (i, kind)
            d = O.hamming64(O.hash_image(T.crop(lossy, box))[0], own)
            print(f"picture {i} {px.shape[1]}x{px.shape[0]} {kind}: box {box} placed {placed}, {d} bits")
            worst = max(worst, d)
            assert d <= T.THRESHOLD, (i, kind, d)
    print(f"largest distance of a JPEG copy's trimmed pHash from its original's pHash: {worst}")
    assert worst == JPEG_WORST                # the docstring's figure is the measured one


def test_two_canvases_of_one_drawing():
    d = T.drawing(T.SEED + 50, 150, 110)
    a, b = T.place(d, 256, 200, 60, 20, (255, 255, 255)), T.place(d, 190, 256, 11, 97, (255, 255, 255))
    assert O.hamming64(O.hash_image(a)[0], O.hash_image(b)[0]) > T.THRESHOLD
    ha, hb = (O.hash_image(T.crop(p, T.pillow_box(p, T.TOLERANCE)))[0] for p in (a, b))
    assert ha == hb == O.hash_image(d)[0]


# ---- trimmed_edges and find_trimmed_duplicates against the oracle's scan ----------------------------------------------------
@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.delenv("KE_DUP_BUCKET_PAIR_CAP", raising=False)
    c = T.OracleScanContext()
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": c)
    return c


def _file(fid, phash, size=1000):
    return DuplicateFile(fid, Path(f"lib/f{fid:04d}.png"), size, 100, 100, int(phash) & MASK)


def _bits(*positions):
    v = 0
    for p in positions:
        v |= 1 << p
    return v


def _table(rng, n):
    """n files with random stored hashes, random trimmed hashes and boxes: nothing matches by chance."""
    h = rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    files = [_file(10 + i, int(h[i, 0])) for i in range(n)]
    boxes = np.array([[i, i + 1, i + 50, i + 60] for i in range(n)], np.int32)
    return files, h[:, 1].copy(), boxes


def _scanner(**kw):
    return DuplicateScanner(DuplicateScanConfig(hamming_threshold=T.THRESHOLD, **kw))


def test_the_table_is_stored_hashes_then_the_trimmed_hashes_of_the_files_with_one(ctx):
    rng = np.random.default_rng(1)
    files, t, boxes = _table(rng, 6)
    has = np.array([True, False, True, True, False, True])
    files[4] = _file(14, files[4].phash, size=77)
    files[5] = _file(15, files[5].phash, size=55)
    assert _scanner(size_ratio=0.5).trimmed_edges(files, t, has, boxes) == []
    call = ctx.calls[-1]
    assert (call["n"], call["first_new"], call["cross"]) == (6 + 4, 6, False)
    assert call["hashes"].tolist() == [f.phash for f in files] + [int(t[i]) for i in (0, 2, 3, 5)]
    assert call["ids"].tolist() == [10, 11, 12, 13, 14, 15, 10, 12, 13, 15]
    assert call["sizes"].tolist() == [1000, 1000, 1000, 1000, 77, 55, 1000, 1000, 1000, 55]
    assert _scanner().trimmed_edges(files, t, np.zeros(6, bool), boxes) == [] and len(ctx.calls) == 1       # nothing trimmed: no scan


def test_a_trimmed_entry_meets_a_stored_hash_and_another_trimmed_entry(ctx):
    rng = np.random.default_rng(2)
    files, t, boxes = _table(rng, 6)
    has = np.array([True, True, True, False, True, True])
    t[1] = np.uint64((files[0].phash ^ _bits(3, 40)) & MASK)            # file 11 cut to its box looks like file 10 as it is
    t[4] = np.uint64(int(t[2]) ^ _bits(63))                               # files 12 and 14: different margins round one picture
    t[3] = np.uint64(files[5].phash)                                     # file 13 has no qualifying box: must not be read
    got = _scanner().trimmed_edges(files, t, has, boxes)
    assert got == [TrimmedMatch(10, 11, False, True, 2, None, (1, 2, 51, 61)),
                   TrimmedMatch(12, 14, True, True, 1, (2, 3, 52, 62), (4, 5, 54, 64))]
    assert _scanner().trimmed_edges(files, t, has) == [TrimmedMatch(10, 11, False, True, 2), TrimmedMatch(12, 14, True, True, 1)]


def test_one_match_per_pair_smallest_hamming_then_the_sides_in_order(ctx):
    rng = np.random.default_rng(3)
    files, t, boxes = _table(rng, 5)
    has = np.ones(5, bool)
    t[0] = np.uint64((files[2].phash ^ _bits(30, 31)) & MASK)            # 10 trimmed against 12 plain: 2 bits
    t[2] = np.uint64(int(t[0]) ^ _bits(5))                                # 10 trimmed against 12 trimmed: 1 bit, wins
    t[1] = np.uint64((files[4].phash ^ _bits(50)) & MASK)                # 11 trimmed against 14 plain: (True, False), 1 bit
    t[4] = np.uint64((files[1].phash ^ _bits(51)) & MASK)                # 11 plain against 14 trimmed: (False, True), 1 bit, first in order
    got = _scanner().trimmed_edges(files, t, has, boxes)
    assert got == [TrimmedMatch(10, 12, True, True, 1, (0, 1, 50, 60), (2, 3, 52, 62)),
                   TrimmedMatch(11, 14, False, True, 1, None, (4, 5, 54, 64))]


def test_a_file_against_its_own_crop_and_a_file_listed_twice_are_dropped(ctx):
    rng = np.random.default_rng(4)
    files, t, boxes = _table(rng, 4)
    t[2] = np.uint64(files[2].phash)                                     # a thin trim: the crop hashes as the file
    files[3] = DuplicateFile(files[1].file_id, files[1].path, 1000, 100, 100, files[1].phash)
    t[3] = np.uint64(files[1].phash)
    assert _scanner().trimmed_edges(files, t, np.ones(4, bool), boxes) == []


def test_size_ratio_applies_to_a_trimmed_entry_through_its_file(ctx):
    rng = np.random.default_rng(5)
    files, t, boxes = _table(rng, 3)
    files[2] = _file(12, files[2].phash, size=100)
    t[2] = np.uint64(files[0].phash)
    has = np.ones(3, bool)
    assert _scanner(size_ratio=0.5).trimmed_edges(files, t, has, boxes) == []
    assert _scanner(size_ratio=0.05).trimmed_edges(files, t, has, boxes) == [TrimmedMatch(10, 12, False, True, 0, None, (2, 3, 52, 62))]


def test_find_trimmed_duplicates_joins_plain_edges_and_matches(ctx, monkeypatch):
    rng = np.random.default_rng(6)
    files, t, boxes = _table(rng, 7)
    files[1] = _file(11, files[0].phash ^ _bits(20))                     # a plain near-duplicate of file 10
    t[4] = np.uint64(files[0].phash ^ _bits(21, 22))                     # file 14 cut to its box looks like file 10
    t[5] = np.uint64(int(t[6]))                                          # files 15 and 16: one picture, two margins
    has, ok = np.ones(7, bool), np.ones(7, bool)
    has[2] = False
    ok[3] = False
    t[3] = np.uint64(files[2].phash)                                     # not ok: must not be read
    seen = {}

    def fake_signatures(paths, *, tolerance=48, device=0):
        seen["paths"], seen["tolerance"] = [str(p) for p in paths], tolerance
        return t, boxes, has, ok

    monkeypatch.setattr(trimmed, "trimmed_signatures", fake_signatures)
    clusters, matches = api.find_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD, tolerance=40)
    assert seen == {"paths": [str(f.path) for f in files], "tolerance": 40}
    assert matches == [TrimmedMatch(10, 14, False, True, 2, None, (4, 5, 54, 64)), TrimmedMatch(11, 14, False, True, 3, None, (4, 5, 54, 64)),
                       TrimmedMatch(15, 16, True, True, 0, (5, 6, 55, 65), (6, 7, 56, 66))]
    assert sorted(sorted(e.file.file_id for e in c.files) for c in clusters) == [[10, 11, 14], [15, 16]]
    plain = api.find_duplicates(files, hamming_threshold=T.THRESHOLD)
    assert sorted(sorted(e.file.file_id for e in c.files) for c in plain) == [[10, 11]]
    assert cli.boxes_of_matches(matches) == {14: (4, 5, 54, 64), 15: (5, 6, 55, 65), 16: (6, 7, 56, 66)}


@pytest.mark.parametrize("other", [dict(turned=True), dict(added_like="%/new/%"), dict(refine=True)])
def test_trimmed_is_refused_with_the_other_modes(other):
    with pytest.raises(ValueError, match="--trimmed cannot be combined"):
        cli.scan_database("no-such.db", trimmed=True, **other)


def test_the_tolerance_must_be_a_byte():
    with pytest.raises(ValueError):
        trimmed.trimmed_signatures(["x.png"], tolerance=256)
