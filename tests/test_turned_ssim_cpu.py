"""The SSIM re-check of turned pairs without a GPU: find_turned_duplicates' bookkeeping, with the scan, the turned
signatures and refine.refine_turned_pairs replaced by stand-ins -- which (pair, orientation) rows are offered, the
either-passes rule, dropped unreadable pairs, the ``ssim`` on the surviving matches, ``orientations_to_keeper`` on the
survivors, ``--turned-ssim`` without ``--turned``, and ``ssim_threshold=None`` calling no refine at all."""
from __future__ import annotations

import sqlite3
from pathlib import Path

import numpy as np
import pytest

from kobato_eyes_amd import api, cli, refine, turned
from kobato_eyes_amd.refine import RefinedMatch
from kobato_eyes_amd.scanner import DuplicateEdge, DuplicateFile, DuplicateScanner, TurnedMatch

# files 10..17.  Plain candidate edges and turned matches as the scan would report them:
PLAIN = {(10, 11): 1, (12, 13): 2, (14, 15): 3}
MATCHES = [TurnedMatch(10, 12, 1, 2), TurnedMatch(12, 13, 5, 0), TurnedMatch(14, 15, 6, 1), TurnedMatch(16, 17, 7, 4), TurnedMatch(11, 16, 3, 5)]
# what the re-check says of (a, b, orientation): a score, or None for a pair with an unreadable file
SCORES = {
    (10, 11, 0): 0.97,          # plain edge passes
    (12, 13, 0): 0.30,          # plain edge fails ...
    (12, 13, 5): 0.95,          # ... but the same pair passes through its turn: stays linked
    (14, 15, 0): 0.93,          # plain edge passes ...
    (14, 15, 6): 0.25,          # ... its turned match does not: linked, but the match is gone
    (10, 12, 1): 0.99,
    (16, 17, 7): None,          # unreadable: dropped
    (11, 16, 3): 0.41,          # the decoy
}


def _files():
    return [DuplicateFile(fid, Path(f"lib/f{fid}.png"), 1000, 100, 100, fid * 0x0123456789ABCDEF & ((1 << 64) - 1)) for fid in range(10, 18)]


@pytest.fixture
def stubs(monkeypatch):
    calls = []

    def fake_refine(pairs, *, thresholds=None, device=0, **kwargs):
        calls.append(([tuple(p) for p in pairs], thresholds.ssim, device))
        out = []
        for a, b, pa, pb, k in pairs:
            assert (str(pa), str(pb)) == (f"lib/f{a}.png", f"lib/f{b}.png")
            score = SCORES[(a, b, k)]
            out.append(None if score is None else RefinedMatch(a, b, score, None, score >= thresholds.ssim, "stub"))
        return out

    monkeypatch.setattr(turned, "turned_signatures", lambda paths, *, device=0: (np.zeros((len(paths), 8), np.uint64), np.ones(len(paths), bool)))
    monkeypatch.setattr(DuplicateScanner, "candidate_edges", lambda self, candidates, first_new=0: {k: DuplicateEdge(k[0], k[1], h) for k, h in PLAIN.items()})
    monkeypatch.setattr(DuplicateScanner, "turned_edges", lambda self, candidates, hashes, ok=None: list(MATCHES))
    monkeypatch.setattr(refine, "refine_turned_pairs", fake_refine)
    return calls


def _groups(clusters):
    return sorted(sorted(e.file.file_id for e in c.files) for c in clusters)


def test_without_a_threshold_nothing_is_refined(stubs):
    clusters, matches = api.find_turned_duplicates(_files())
    assert stubs == []
    assert matches == MATCHES and all(m.ssim is None for m in matches)
    assert _groups(clusters) == [[10, 11, 12, 13, 16, 17], [14, 15]]
    assert TurnedMatch(1, 2, 3, 4) == TurnedMatch(1, 2, 3, 4, None)        # the new field has a default


def test_the_rows_offered_and_what_survives(stubs):
    clusters, matches = api.find_turned_duplicates(_files(), ssim_threshold=0.9, device=3)
    assert len(stubs) == 1                                                 # one call for the plain edges and the matches together
    rows, threshold, device = stubs[0]
    assert (threshold, device) == (0.9, 3)
    want_rows = [(a, b, Path(f"lib/f{a}.png"), Path(f"lib/f{b}.png"), 0) for a, b in PLAIN]
    want_rows += [(m.file_id_a, m.file_id_b, Path(f"lib/f{m.file_id_a}.png"), Path(f"lib/f{m.file_id_b}.png"), m.orientation) for m in MATCHES]
    assert rows == want_rows
    # the surviving matches, each with its score; 16-17 (unreadable), 11-16 (the decoy) and 14-15's turn are gone
    assert matches == [TurnedMatch(10, 12, 1, 2, 0.99), TurnedMatch(12, 13, 5, 0, 0.95)]
    # 12-13 failed as a plain edge and passed as a match: linked; 14-15 the other way round: linked
    assert _groups(clusters) == [[10, 11, 12, 13], [14, 15]]


def test_threshold_zero_keeps_what_could_be_read(stubs):
    clusters, matches = api.find_turned_duplicates(_files(), ssim_threshold=0.0)
    assert [(m.file_id_a, m.file_id_b) for m in matches] == [(10, 12), (12, 13), (14, 15), (11, 16)]
    assert [m.ssim for m in matches] == [0.99, 0.95, 0.25, 0.41]
    assert _groups(clusters) == [[10, 11, 12, 13, 16], [14, 15]]


def test_orientations_to_keeper_works_on_the_survivors(stubs):
    clusters, matches, plain_keys = api._view_scan("turned", _files(), hamming_threshold=8, size_ratio=None, band_bits=16, band_count=4, device=0,
                                                   ssim_threshold=0.9)
    assert plain_keys == {(10, 11), (14, 15)}                              # 12-13's plain edge did not pass
    orient = cli.orientations_to_keeper(clusters, matches, plain_keys)
    by_members = {tuple(sorted(e.file.file_id for e in c.files)): c for c in clusters}
    assert 14 not in orient and 15 not in orient                           # linked as the pixels lie: the failed turn says nothing
    keeper = by_members[(10, 11, 12, 13)].keeper_id
    # 12 is the mirror of 10 (and so of 11); 13 turned clockwise is 12: relative to 10, COMPOSE[5][1]
    to_10 = {10: 0, 11: 0, 12: 1, 13: turned.COMPOSE[5][1]}
    want = {f: turned.COMPOSE[k][turned.INVERSE[to_10[keeper]]] for f, k in to_10.items()}
    assert {f: orient.get(f, 0) for f in to_10} == want
    # without the re-check the decoy's link and the unreadable pair would have been walked too
    clusters0, matches0, keys0 = api._view_scan("turned", _files(), hamming_threshold=8, size_ratio=None, band_bits=16, band_count=4, device=0)
    assert keys0 == set(PLAIN) and matches0 == MATCHES


def test_turned_ssim_needs_turned(tmp_path, stubs):
    with pytest.raises(ValueError, match="--turned-ssim needs --turned"):
        cli.scan_database(str(tmp_path / "absent.db"), turned_ssim=0.9)
    with pytest.raises(ValueError, match="--turned-ssim needs --turned"):
        cli.main(["scan-dups", "--db", str(tmp_path / "absent.db"), "--turned-ssim", "0.9"])
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
    orient: dict = {}
    clusters = cli.scan_database(db, turned=True, turned_ssim=0.9, orientations_out=orient)
    assert len(stubs) == 1 and stubs[0][1] == 0.9
    assert _groups(clusters) == [[10, 11, 12, 13], [14, 15]]
    assert set(orient) <= {10, 11, 12, 13}
    stubs.clear()
    assert _groups(cli.scan_database(db, turned=True)) == [[10, 11, 12, 13, 16, 17], [14, 15]]
    assert stubs == []
