"""Copies that are both bordered and turned, without a GPU.

* The corpus of _turned_trimmed_cases is what it claims to be, on the CPU oracle alone: every planted copy
  ``turn(k, bordered(original))`` has its best trimmed-turned hash at orientation INVERSE[k], within the scan's threshold of and
  sharing a 16-bit band with its original's stored pHash; neither the oracle's restatement of ``turned_edges`` (stored pHash
  against the seven turned hashes of the whole picture) nor of ``trimmed_edges`` (stored and trimmed pHashes) links any of them
  to its original -- the gap the two existing modes leave; every true copy's box, turned back, scores at least 0.9 against its
  original and every decoy's under 0.5, while the decoy's hash links it.  Conditions on the seeds, not measurements of the
  library.
* The host logic: a table position -> (flags, k), the exchange through INVERSE, the tie-break; ``turned_trimmed_edges``' table
  and what it keeps, with a stand-in scan; ``find_turned_trimmed_duplicates``' bookkeeping with a stand-in refine.
* The CLI's refusals, and the ``ValueError``s of ``refine_turned_trimmed_pairs`` before anything is decoded."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import _trim_cases as T
import _trimmed_ssim_cases as S
import _turned_cases as TC
import _turned_trimmed_cases as V
from kobato_eyes_amd import api, cli, refine, scanner, turned, turned_trimmed
from kobato_eyes_amd._native import EDGE_DTYPE
from kobato_eyes_amd.refine import RefinedMatch
from kobato_eyes_amd.scanner import DuplicateEdge, DuplicateFile, DuplicateScanConfig, DuplicateScanner, TransformedMatch, TrimmedMatch
from oracle import oracle as O


def _links(stored: int, other: int) -> bool:
    """What the banded scan can report: within the threshold and a 16-bit band in common."""
    return O.hamming64(stored, other) <= T.THRESHOLD and S.same_band(stored, other)


# ---- the corpus --------------------------------------------------------------------------------------------------------------
def test_the_corpus_is_what_it_claims_to_be(tmp_path):
    from PIL import Image

    records = V.write_corpus(tmp_path)
    assert len(records) == (4 + 16 + 2) + len(V.PLANTED) + 3 * len(TC.PLANTED) + len(V.DECOY_TURNS)
    assert [r["file_id"] for r in records] == list(range(1, len(records) + 1))
    opened = {r["file_id"]: np.asarray(Image.open(r["path"]).convert("RGB")) for r in records}
    original = V.original_of(records)
    planted = [r for r in records if r["planted"]]
    assert {r["orientation"] for r in planted} == set(range(1, 8)) and {r["kind"] for r in planted} == set(T.BORDER_KINDS)
    assert {Path(r["path"]).suffix for r in planted} == {".png", ".jpg"}
    assert any(r["orientation"] == 0 and r["kind"] in T.BORDER_KINDS for r in records)          # orientation-0 matches are present
    assert any(r["family"][0] == "turn" and r["orientation"] for r in records)                   # and unboxed ones
    lowest = 1.0
    for r in records:
        if not (r["planted"] or r["decoy"]):
            continue
        k = r["orientation"]
        px, own = opened[r["file_id"]], opened[original[r["family"]]]
        stored_own, stored_px = O.hash_image(own)[0], O.hash_image(px)[0]
        box, hashes = V.trimmed_turned_hashes(px)
        assert hashes is not None, r
        distances = [O.hamming64(stored_own, h) for h in hashes]
        best = int(np.argmin(distances))
        back = V.view(px, box, turned.INVERSE[k])
        score = O.ssim_fit(own, back)
        print(f"{Path(r['path']).name}: box {box}, distances {distances}, ssim of the box turned back {score:.4f}")
        assert best == turned.INVERSE[k] and distances.count(distances[best]) == 1, r
        assert _links(stored_own, hashes[best]), r
        if r["decoy"]:
            assert np.array_equal(px, V.decoy_picture(r["family"][1]))
            assert score < 0.5, r
            continue
        lowest = min(lowest, score)
        assert score >= V.SSIM_THRESHOLD, r
        # the gap: the two existing modes, restated on the oracle, link this copy to its original through nothing
        assert not _links(stored_own, stored_px), r
        whole_own, whole_px = V.turned_hashes(own), V.turned_hashes(px)
        assert not any(_links(stored_own, h) for h in whole_px[1:]) and not any(_links(stored_px, h) for h in whole_own[1:]), r
        _, cut_own = V.trimmed_turned_hashes(own)
        assert not _links(stored_own, hashes[0]), r                              # stored x trimmed
        if cut_own is not None:                                                  # trimmed x stored, trimmed x trimmed
            assert not _links(stored_px, cut_own[0]) and not _links(cut_own[0], hashes[0]), r
    print(f"lowest score of a true copy's box, turned back: {lowest:.4f}")


# ---- table positions, the exchange, the tie-break ---------------------------------------------------------------------------------
def test_a_table_position_decodes_to_flags_and_an_orientation():
    n, trimmed_rows, turned_rows = 5, [1, 4], [0, 2, 3]
    # first part: 0..4 stored, 5..6 the trimmed pHash of candidates 1 and 4; second part from 7: 3 x 7 turned, then 2 x 7 of crops
    assert scanner.view_edge(3, 7, n, trimmed_rows, turned_rows) == (3, False, 0, False, 1)
    assert scanner.view_edge(3, 7 + 6, n, trimmed_rows, turned_rows) == (3, False, 0, False, 7)
    assert scanner.view_edge(0, 7 + 7, n, trimmed_rows, turned_rows) == (0, False, 2, False, 1)
    assert scanner.view_edge(6, 7 + 20, n, trimmed_rows, turned_rows) == (4, True, 3, False, 7)
    assert scanner.view_edge(5, 7 + 21, n, trimmed_rows, turned_rows) == (1, True, 1, True, 1)
    assert scanner.view_edge(2, 7 + 21 + 7 + 4, n, trimmed_rows, turned_rows) == (2, False, 4, True, 5)
    assert scanner.view_edge(2, 7 + 21 + 13, n, trimmed_rows, turned_rows) == (2, False, 4, True, 7)
    # every position of the second part, once, in table order
    seen = [scanner.view_edge(0, b, n, trimmed_rows, turned_rows)[2:] for b in range(7, 7 + 35)]
    assert seen == [(c, False, k) for c in turned_rows for k in range(1, 8)] + [(c, True, k) for c in trimmed_rows for k in range(1, 8)]


def test_a_match_found_from_the_larger_id_is_exchanged_through_inverse():
    for k in range(8):
        assert scanner.ordered_view(3, True, 9, False, k) == (3, True, 9, False, k)
        assert scanner.ordered_view(9, True, 3, False, k) == (3, False, 9, True, turned.INVERSE[k])
    assert scanner.ordered_view(9, False, 3, True, 5) == (3, True, 9, False, 6)          # the two quarter turns undo each other
    probe = np.arange(6).reshape(2, 3)
    for k in range(8):                                                                   # what the exchange rests on
        assert np.array_equal(turned.turn(turned.INVERSE[k], turned.turn(k, probe)), probe)


def test_the_tie_break():
    rank = scanner.view_rank
    assert rank(3, 5, True, True) < rank(4, 1, False, False)                             # hamming first
    assert rank(3, 1, True, True) < rank(3, 2, False, False)                             # then the orientation
    assert rank(3, 2, False, True) < rank(3, 2, True, False) < rank(3, 2, True, True)    # then the flags, a's first
    assert rank(np.int64(3), np.int32(2), np.bool_(False), True) == (3, 2, False, True)


# ---- turned_trimmed_edges with a stand-in scan ----------------------------------------------------------------------------------
class _Scan:
    def __init__(self, edges):
        self.edges, self.calls = edges, []

    def hamming_scan(self, hashes, n, **kw):
        self.calls.append(dict(hashes=np.array(hashes), n=n, **kw))
        raw = np.zeros(len(self.edges), EDGE_DTYPE)
        for i, (a, b, h) in enumerate(self.edges):
            raw[i]["a"], raw[i]["b"], raw[i]["h"] = a, b, h
        return raw, np.zeros(4, np.uint64)


def test_turned_trimmed_edges_builds_the_table_and_keeps_the_best_per_pair(monkeypatch):
    ids = [40, 10, 30, 20]
    files = [DuplicateFile(fid, Path(f"f{fid}.png"), 100 * fid, 64, 64, 0x1000 + fid) for fid in ids]
    n = len(files)
    tn = (np.arange(n * 8, dtype=np.uint64) + np.uint64(0x2000)).reshape(n, 8)
    cut = (np.arange(n * 8, dtype=np.uint64) + np.uint64(0x3000)).reshape(n, 8)
    ok, has = np.array([True, True, False, True]), np.array([False, True, True, False])
    boxes = np.array([[0, 0, 0, 0], [1, 2, 31, 42], [3, 4, 53, 64], [0, 0, 0, 0]], np.int32)
    src_o, src_t = [0, 1, 3], [1, 2]
    first_new = n + 2
    second = lambda cand, trimmed, k: first_new + (7 * len(src_o) + 7 * src_t.index(cand) if trimmed else 7 * src_o.index(cand)) + k - 1
    edges = [
        (1, second(0, False, 5), 4),        # stored 10 ~ orientation 5 of 40: found from the smaller id
        (0, second(1, False, 5), 3),        # stored 40 ~ orientation 5 of 10: exchanged, orientation 6, and the better hamming
        (1, second(2, True, 2), 2),         # stored 10 ~ orientation 2 of the crop of 30
        (2, second(1, True, 2), 2),         # stored 30 ~ orientation 2 of the crop of 10: the same hamming and k, flags (True, False)
        (5, second(3, False, 7), 6),        # trimmed 30 ~ orientation 7 of 20: exchanged -> (20, False, 30, True, 7)
        (3, second(2, True, 1), 6),         # stored 20 ~ orientation 1 of the crop of 30: the smaller orientation at the same hamming
    ]
    scan = _Scan(edges)
    monkeypatch.setattr(scanner._native, "get_context", lambda device=0: scan)
    found = DuplicateScanner(DuplicateScanConfig(hamming_threshold=7, size_ratio=0.5), device=2, part_index=1, part_count=3) \
        .turned_trimmed_edges(files, tn, cut, has, ok, boxes)
    call = scan.calls[0]
    want_table = np.concatenate([np.array([0x1000 + i for i in ids], np.uint64), cut[src_t, 0], tn[src_o, 1:8].reshape(-1),
                                 cut[src_t, 1:8].reshape(-1)])
    assert np.array_equal(call["hashes"], want_table) and call["n"] == len(want_table) == n + 2 + 21 + 14
    assert call["first_new"] == first_new and call["cross"] is True
    rows = list(range(n)) + src_t + [c for c in src_o for _ in range(7)] + [c for c in src_t for _ in range(7)]
    assert call["ids"].tolist() == [ids[c] for c in rows] and call["sizes"].tolist() == [100 * ids[c] for c in rows]
    assert (call["threshold"], call["size_ratio"], call["part_index"], call["part_count"]) == (7, 0.5, 1, 3)
    assert found == [
        TransformedMatch(10, 30, False, True, 2, 2, None, (3, 4, 53, 64)),   # (2, 2, False, True) < (2, 2, True, False)
        TransformedMatch(10, 40, False, False, 6, 3),
        TransformedMatch(20, 30, False, True, 1, 6, None, (3, 4, 53, 64)),
    ]
    # the second edge of 10-30 alone: stored 30 against the crop of 10, seen from 10's side
    scan.edges = [edges[3]]
    assert DuplicateScanner(DuplicateScanConfig()).turned_trimmed_edges(files, tn, cut, has, ok, boxes) == \
        [TransformedMatch(10, 30, True, False, 2, 2, (1, 2, 31, 42), None)]
    # nothing to scan
    assert DuplicateScanner(DuplicateScanConfig()).turned_trimmed_edges(files, tn, cut, np.zeros(n, bool), np.zeros(n, bool)) == []


# ---- find_turned_trimmed_duplicates with a stand-in refine -------------------------------------------------------------------------
PLAIN = {(10, 11): 1, (12, 13): 2, (14, 15): 3}
BOX = (4, 5, 54, 64)
TRIMMED = [TrimmedMatch(10, 12, False, True, 2, None, BOX), TrimmedMatch(12, 13, True, True, 3, BOX, BOX)]
VIEWED = [TransformedMatch(12, 13, True, True, 5, 1, BOX, BOX), TransformedMatch(14, 15, False, True, 3, 1, None, BOX),
          TransformedMatch(16, 17, True, False, 6, 4, BOX, None), TransformedMatch(11, 16, True, True, 2, 5, BOX, BOX),
          TransformedMatch(10, 12, True, True, 1, 2, BOX, BOX)]
# the best per pair: 10-12 keeps the orientation-0 match (same hamming, smaller orientation), 12-13 the turned one (smaller hamming)
MATCHES = [TransformedMatch(10, 12, False, True, 0, 2, None, BOX), VIEWED[3], VIEWED[0], VIEWED[1], VIEWED[2]]
SCORES = {
    (10, 11, False, False, 0): 0.97,      # plain edge passes
    (12, 13, False, False, 0): 0.30,      # plain edge fails ...
    (12, 13, True, True, 5): 0.95,        # ... but the same pair passes cut and turned: stays linked
    (14, 15, False, False, 0): 0.93,      # plain edge passes ...
    (14, 15, False, True, 3): 0.25,       # ... its match does not: linked, but the match is gone
    (10, 12, False, True, 0): 0.99,
    (16, 17, True, False, 6): None,       # unreadable: dropped
    (11, 16, True, True, 2): 0.41,        # the decoy
}


def _files():
    return [DuplicateFile(fid, Path(f"lib/f{fid}.png"), 1000, 100, 100, fid * 0x0123456789ABCDEF & ((1 << 64) - 1)) for fid in range(10, 18)]


@pytest.fixture
def stubs(monkeypatch):
    calls = []

    def fake_refine(pairs, *, tolerance=48, thresholds=None, device=0, **kwargs):
        calls.append(([tuple(p) for p in pairs], thresholds.ssim, device, tolerance))
        out = []
        for a, b, pa, pb, ta, tb, k in pairs:
            assert (str(pa), str(pb)) == (f"lib/f{a}.png", f"lib/f{b}.png")
            score = SCORES[(a, b, ta, tb, k)]
            out.append(None if score is None else RefinedMatch(a, b, score, None, score >= thresholds.ssim, "stub"))
        return out

    n = len(_files())
    monkeypatch.setattr(turned_trimmed, "turned_trimmed_signatures", lambda paths, *, tolerance=48, device=0: (
        np.zeros((n, 8), np.uint64), np.zeros((n, 8), np.uint64), np.zeros((n, 4), np.int32), np.ones(n, bool), np.ones(n, bool)))
    monkeypatch.setattr(DuplicateScanner, "candidate_edges", lambda self, candidates, first_new=0: {k: DuplicateEdge(k[0], k[1], h) for k, h in PLAIN.items()})
    monkeypatch.setattr(DuplicateScanner, "trimmed_edges", lambda self, candidates, hashes, has, boxes=None: list(TRIMMED))
    monkeypatch.setattr(DuplicateScanner, "turned_trimmed_edges", lambda self, candidates, tn, cut, has, ok=None, boxes=None: list(VIEWED))
    monkeypatch.setattr(refine, "refine_turned_trimmed_pairs", fake_refine)
    return calls


def _groups(clusters):
    return sorted(sorted(e.file.file_id for e in c.files) for c in clusters)


def test_without_a_threshold_the_best_match_per_pair_and_nothing_refined(stubs):
    clusters, matches = api.find_turned_trimmed_duplicates(_files())
    assert stubs == []
    assert matches == MATCHES and all(m.ssim is None for m in matches)
    assert _groups(clusters) == [[10, 11, 12, 13, 16, 17], [14, 15]]


def test_the_rows_offered_and_what_survives(stubs):
    clusters, matches = api.find_turned_trimmed_duplicates(_files(), ssim_threshold=0.9, tolerance=40, device=3)
    assert len(stubs) == 1                                                 # one call for the plain edges and the matches together
    rows, threshold, device, tolerance = stubs[0]
    assert (threshold, device, tolerance) == (0.9, 3, 40)
    want_rows = [(a, b, Path(f"lib/f{a}.png"), Path(f"lib/f{b}.png"), False, False, 0) for a, b in PLAIN]
    want_rows += [(m.file_id_a, m.file_id_b, Path(f"lib/f{m.file_id_a}.png"), Path(f"lib/f{m.file_id_b}.png"), m.trimmed_a, m.trimmed_b,
                   m.orientation) for m in MATCHES]
    assert rows == want_rows
    assert matches == [TransformedMatch(10, 12, False, True, 0, 2, None, BOX, 0.99), TransformedMatch(12, 13, True, True, 5, 1, BOX, BOX, 0.95)]
    # 12-13 failed as a plain edge and passed as a match: linked; 14-15 the other way round: linked
    assert _groups(clusters) == [[10, 11, 12, 13], [14, 15]]
    assert cli.boxes_of_matches(matches) == {12: BOX, 13: BOX}
    # from the keeper outwards: 13 reaches its group through the quarter turn alone
    assert set(cli.orientations_to_keeper(clusters, matches, {(10, 11), (14, 15)}).values()) <= {5, 6}


# ---- the CLI's refusals, the seam's ValueErrors -------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", [dict(turned=True), dict(trimmed=True), dict(added_like="%/new/%"), dict(refine=True)])
def test_turned_trimmed_is_a_mode_of_its_own(tmp_path, stubs, other):
    with pytest.raises(ValueError, match="--turned-trimmed cannot be combined"):
        cli.scan_database(str(tmp_path / "absent.db"), turned_trimmed=True, **other)
    flag = {"turned": ["--turned"], "trimmed": ["--trimmed"], "added_like": ["--added-like", "%/new/%"], "refine": ["--refine"]}[next(iter(other))]
    with pytest.raises(ValueError, match="--turned-trimmed cannot be combined"):
        cli.main(["scan-dups", "--db", str(tmp_path / "absent.db"), "--turned-trimmed"] + flag)
    assert stubs == []


def test_turned_trimmed_ssim_needs_the_mode_and_the_two_old_modes_still_refuse_each_other(tmp_path, stubs):
    with pytest.raises(ValueError, match="--turned-trimmed-ssim needs --turned-trimmed"):
        cli.scan_database(str(tmp_path / "absent.db"), turned_trimmed_ssim=0.9)
    with pytest.raises(ValueError, match="--turned-trimmed-ssim needs --turned-trimmed"):
        cli.main(["scan-dups", "--db", str(tmp_path / "absent.db"), "--turned-trimmed-ssim", "0.9", "--turned"])
    with pytest.raises(ValueError, match="--trimmed cannot be combined"):                # today's message stays
        cli.main(["scan-dups", "--db", str(tmp_path / "absent.db"), "--trimmed", "--turned"])
    assert stubs == []


def test_the_seam_refuses_before_anything_is_decoded(monkeypatch):
    monkeypatch.setattr(refine._native, "get_context", lambda *a, **k: pytest.fail("a context was asked for"))
    row = (1, 2, "a.png", "b.png", True, False, 3)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="tolerance"):
            refine.refine_turned_trimmed_pairs([row], tolerance=bad)
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="orientation"):
            refine.refine_turned_trimmed_pairs([row, row[:6] + (bad,)])
    with pytest.raises(ValueError, match="tolerance"):
        turned_trimmed.turned_trimmed_signatures(["a.png"], tolerance=300)
