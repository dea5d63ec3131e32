"""The SSIM re-check of trimmed pairs without a GPU.

* The preconditions of tests/test_gpu_trimmed_ssim.py's end-to-end test, on the CPU oracle alone: on the corpus of
  _trimmed_ssim_cases every true bordered copy's content box scores at least 0.9 against its original (the lowest found is
  0.9599, a grey-frame JPEG whose box came out one row too tall), the drawing's two canvases score at least 0.9 box against
  box, and every decoy's box qualifies, lies within the scan's threshold of and shares a band with its original's stored
  pHash, and scores under 0.5.  Conditions on the seeds, not measurements of the library.
* find_trimmed_duplicates' bookkeeping, with the scan, the trimmed signatures and refine.refine_trimmed_pairs replaced by
  stand-ins: which (pair, trimmed_a, trimmed_b) rows are offered, the either-passes rule, dropped unreadable pairs, the
  ``ssim`` on the surviving matches, and ``ssim_threshold=None`` calling no refine at all.
* ``--trimmed-ssim`` without ``--trimmed``; a tolerance that is no byte."""
from __future__ import annotations

import sqlite3
from pathlib import Path

import numpy as np
import pytest

import _trim_cases as T
import _trimmed_ssim_cases as S
from kobato_eyes_amd import api, cli, refine, trimmed
from kobato_eyes_amd.refine import RefinedMatch
from kobato_eyes_amd.scanner import DuplicateEdge, DuplicateFile, DuplicateScanner, TrimmedMatch
from oracle import oracle as O


# ---- the preconditions of the GPU test --------------------------------------------------------------------------------------
def test_true_copies_score_high_on_their_boxes_and_decoys_low(tmp_path):
    from PIL import Image

    records = S.write_corpus(tmp_path)
    assert len(records) == 4 + 16 + 2 + 4
    opened = {r["file_id"]: np.asarray(Image.open(r["path"]).convert("RGB")) for r in records}
    original = {r["original"]: r["file_id"] for r in records if r["kind"] is None}
    lowest = 1.0
    for r in records:
        if r["kind"] is None or r["original"] == "drawing":
            continue
        px, own = opened[r["file_id"]], opened[original[r["original"]]]
        box = T.content_box(px, T.TOLERANCE)
        score = O.ssim_fit(own, T.crop(px, box))
        print(f"{Path(r['path']).name}: box {box}, ssim {score:.4f} (the whole file: {O.ssim_fit(own, px):.4f})")
        if not r["decoy"]:
            lowest = min(lowest, score)
            assert score >= S.SSIM_THRESHOLD, r
            continue
        assert np.array_equal(px, S.decoy_picture(r["original"]))
        assert T.qualifies(px.shape[1], px.shape[0], box), r
        cut, stored = O.hash_image(T.crop(px, box))[0], O.hash_image(own)[0]
        assert O.hamming64(cut, stored) <= T.THRESHOLD and S.same_band(cut, stored), r
        assert score < 0.5, r
    print(f"lowest score of a true copy's box: {lowest:.4f}")
    a, b = (opened[r["file_id"]] for r in records if r["original"] == "drawing")
    both = O.ssim_fit(T.crop(a, T.content_box(a, T.TOLERANCE)), T.crop(b, T.content_box(b, T.TOLERANCE)))
    assert both >= S.SSIM_THRESHOLD


# ---- find_trimmed_duplicates with a stub refine -----------------------------------------------------------------------------------
# files 10..17.  Plain candidate edges and trimmed matches as the scan would report them:
PLAIN = {(10, 11): 1, (12, 13): 2, (14, 15): 3}
BOX = (4, 5, 54, 64)
MATCHES = [TrimmedMatch(10, 12, False, True, 2, None, BOX), TrimmedMatch(12, 13, True, True, 0, BOX, BOX),
           TrimmedMatch(14, 15, True, False, 1, BOX, None), TrimmedMatch(16, 17, False, True, 4, None, BOX),
           TrimmedMatch(11, 16, True, True, 5, BOX, BOX)]
# what the re-check says of (a, b, trimmed_a, trimmed_b): a score, or None for a pair with an unreadable file
SCORES = {
    (10, 11, False, False): 0.97,         # plain edge passes
    (12, 13, False, False): 0.30,         # plain edge fails ...
    (12, 13, True, True): 0.95,           # ... but the same pair passes on its boxes: stays linked
    (14, 15, False, False): 0.93,         # plain edge passes ...
    (14, 15, True, False): 0.25,          # ... its trimmed match does not: linked, but the match is gone
    (10, 12, False, True): 0.99,
    (16, 17, False, True): None,          # unreadable: dropped
    (11, 16, True, True): 0.41,           # the decoy
}


def _files():
    return [DuplicateFile(fid, Path(f"lib/f{fid}.png"), 1000, 100, 100, fid * 0x0123456789ABCDEF & ((1 << 64) - 1)) for fid in range(10, 18)]


@pytest.fixture
def stubs(monkeypatch):
    calls = []

    def fake_refine(pairs, *, tolerance=48, thresholds=None, device=0, **kwargs):
        calls.append(([tuple(p) for p in pairs], thresholds.ssim, device, tolerance))
        out = []
        for a, b, pa, pb, ta, tb in pairs:
            assert (str(pa), str(pb)) == (f"lib/f{a}.png", f"lib/f{b}.png")
            score = SCORES[(a, b, ta, tb)]
            out.append(None if score is None else RefinedMatch(a, b, score, None, score >= thresholds.ssim, "stub"))
        return out

    n = len(_files())
    monkeypatch.setattr(trimmed, "trimmed_signatures", lambda paths, *, tolerance=48, device=0: (
        np.zeros(n, np.uint64), np.zeros((n, 4), np.int32), np.ones(n, bool), np.ones(n, bool)))
    monkeypatch.setattr(DuplicateScanner, "candidate_edges", lambda self, candidates, first_new=0: {k: DuplicateEdge(k[0], k[1], h) for k, h in PLAIN.items()})
    monkeypatch.setattr(DuplicateScanner, "trimmed_edges", lambda self, candidates, hashes, has, boxes=None: list(MATCHES))
    monkeypatch.setattr(refine, "refine_trimmed_pairs", fake_refine)
    return calls


def _groups(clusters):
    return sorted(sorted(e.file.file_id for e in c.files) for c in clusters)


def test_without_a_threshold_nothing_is_refined(stubs):
    clusters, matches = api.find_trimmed_duplicates(_files())
    assert stubs == []
    assert matches == MATCHES and all(m.ssim is None for m in matches)
    assert _groups(clusters) == [[10, 11, 12, 13, 16, 17], [14, 15]]
    assert TrimmedMatch(1, 2, True, False, 3, BOX) == TrimmedMatch(1, 2, True, False, 3, BOX, None, None)      # the new field is last and has a default


def test_the_rows_offered_and_what_survives(stubs):
    clusters, matches = api.find_trimmed_duplicates(_files(), ssim_threshold=0.9, tolerance=40, device=3)
    assert len(stubs) == 1                                                 # one call for the plain edges and the matches together
    rows, threshold, device, tolerance = stubs[0]
    assert (threshold, device, tolerance) == (0.9, 3, 40)
    want_rows = [(a, b, Path(f"lib/f{a}.png"), Path(f"lib/f{b}.png"), False, False) for a, b in PLAIN]
    want_rows += [(m.file_id_a, m.file_id_b, Path(f"lib/f{m.file_id_a}.png"), Path(f"lib/f{m.file_id_b}.png"), m.trimmed_a, m.trimmed_b)
                  for m in MATCHES]
    assert rows == want_rows
    # the surviving matches, each with its score; 16-17 (unreadable), 11-16 (the decoy) and 14-15's crop are gone
    assert matches == [TrimmedMatch(10, 12, False, True, 2, None, BOX, 0.99), TrimmedMatch(12, 13, True, True, 0, BOX, BOX, 0.95)]
    # 12-13 failed as a plain edge and passed as a match: linked; 14-15 the other way round: linked
    assert _groups(clusters) == [[10, 11, 12, 13], [14, 15]]
    assert cli.boxes_of_matches(matches) == {12: BOX, 13: BOX}


def test_threshold_zero_keeps_what_could_be_read(stubs):
    clusters, matches = api.find_trimmed_duplicates(_files(), ssim_threshold=0.0)
    assert [(m.file_id_a, m.file_id_b) for m in matches] == [(10, 12), (12, 13), (14, 15), (11, 16)]
    assert [m.ssim for m in matches] == [0.99, 0.95, 0.25, 0.41]
    assert [(m.trimmed_a, m.trimmed_b, m.hamming, m.box_a, m.box_b) for m in matches] == \
        [(m.trimmed_a, m.trimmed_b, m.hamming, m.box_a, m.box_b) for m in MATCHES if (m.file_id_a, m.file_id_b) != (16, 17)]
    assert _groups(clusters) == [[10, 11, 12, 13, 16], [14, 15]]


def test_trimmed_ssim_needs_trimmed(tmp_path, stubs):
    with pytest.raises(ValueError, match="--trimmed-ssim needs --trimmed"):
        cli.scan_database(str(tmp_path / "absent.db"), trimmed_ssim=0.9)
    with pytest.raises(ValueError, match="--trimmed-ssim needs --trimmed"):
        cli.main(["scan-dups", "--db", str(tmp_path / "absent.db"), "--trimmed-ssim", "0.9"])
    assert stubs == []


def test_scan_database_hands_the_threshold_on(tmp_path, stubs):
    db = str(tmp_path / "k.db")
    conn = sqlite3.connect(db)
    conn.execute("CREATE TABLE files (id INTEGER PRIMARY KEY, path TEXT, size INTEGER, width INTEGER, height INTEGER, is_present INTEGER)")
    conn.execute("CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER, dhash_u64 INTEGER)")
    for f in _files():
        conn.execute("INSERT INTO files VALUES (?, ?, ?, ?, ?, 1)", (f.file_id, str(f.path), f.size, f.width, f.height))
        conn.execute("INSERT INTO signatures VALUES (?, ?, 0)", (f.file_id, f.phash - (1 << 64) if f.phash >= 1 << 63 else f.phash))
    conn.commit()
    conn.close()
    boxes: dict = {}
    clusters = cli.scan_database(db, trimmed=True, trimmed_ssim=0.9, trim_tolerance=33, boxes_out=boxes)
    assert len(stubs) == 1 and stubs[0][1] == 0.9 and stubs[0][3] == 33
    assert _groups(clusters) == [[10, 11, 12, 13], [14, 15]]
    assert boxes == {12: BOX, 13: BOX}                                     # of the survivors
    stubs.clear()
    assert _groups(cli.scan_database(db, trimmed=True)) == [[10, 11, 12, 13, 16, 17], [14, 15]]
    assert stubs == []


def test_the_tolerance_must_be_a_byte_before_anything_is_decoded(monkeypatch):
    monkeypatch.setattr(refine._native, "get_context", lambda *a, **k: pytest.fail("a context was asked for"))
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="tolerance"):
            refine.refine_trimmed_pairs([(1, 2, "a.png", "b.png", True, False)], tolerance=bad)
