"""The exact scan's host side without a GPU: DuplicateScanner, the api calls and the CLI flag under ``exact``, held to the
NumPy definition of tests/_scan_exact_cases.py through a stand-in context that answers ``exact=True`` from it.

The table (``_scan_exact_cases.table``) is bases and copies with 0..14 flipped bits, a good share of the copies with a flipped
bit in every 16-bit band: within the threshold, and invisible to the banded scan.  The recall tests plant such pairs by name
and show that ``exact=True`` links them and the default provably does not."""
from __future__ import annotations

import dataclasses
import logging
import os
import sqlite3
from pathlib import Path

import numpy as np
import pytest

import _scan_exact_cases as X
from kobato_eyes_amd import _native, api, cli, ranks, trimmed, turned, turned_trimmed
from kobato_eyes_amd.scanner import (DuplicateEdge, DuplicateFile, DuplicateScanConfig, DuplicateScanner, TurnedMatch,
                                     assemble_clusters)
from oracle import oracle as O

T = X.THRESHOLD
MASK = (1 << 64) - 1
N = 240
H, IDS, SIZES = X.table(N)
UNIQUE = np.arange(N, dtype=np.int64) * 3 + 11            # the table's ids without the repeats


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.delenv("KE_DUP_BUCKET_PAIR_CAP", raising=False)
    c = X.ExactScanContext()
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": c)
    return c


def _files(h=H, ids=UNIQUE, sizes=None):
    return [DuplicateFile(int(ids[i]), Path(f"lib/f{i:04d}.png"), int(sizes[i]) if sizes is not None else 1000 + i, 100, 100, int(h[i]))
            for i in range(len(h))]


def _want_edges(rows, ids):
    """Definition rows over a table of unique ids -> the {(id_lo, id_hi): hamming} the scanner must end up with."""
    return {tuple(sorted((int(ids[a]), int(ids[b])))): int(h) for a, b, h, _ in rows}


def _groups(clusters):
    return sorted(sorted(e.file.file_id for e in c.files) for c in clusters)


def _clusters_of(files, rows, ids, previous=()):
    edges = [DuplicateEdge(int(ids[a]), int(ids[b]), int(h)) for a, b, h, _ in rows]
    return assemble_clusters(files, edges, previous=previous) if edges or previous else []


def _same_clusters(got, want):
    flat = lambda cs: [(c.keeper_id, [(e.file.file_id, e.best_hamming) for e in c.files]) for c in cs]
    return flat(got) == flat(want)


# ---- the definition and the table ---------------------------------------------------------------------------------------
def test_the_tables_pairs_within_the_threshold_are_bandless_for_at_least_a_third():
    for n in (N, 3000):
        within, bandless = X.bandless_share(X.table(n)[0])
        print(n, within, bandless)
        assert within >= n // 4 and 3 * bandless >= within


@pytest.mark.parametrize("region, first_new", [(X.REGION_ALL, 0), (X.REGION_FROM, 100), (X.REGION_CROSS, 100)])
def test_the_definitions_banded_edges_are_the_oracles(region, first_new):
    rows = X.definition(H, ids=IDS, sizes=SIZES, threshold=T, size_ratio=0.5, region=region, first_new=first_new)
    e, _ = O.scan_banded(H, ids=None, sizes=SIZES, threshold=T, size_ratio=0.5)
    e = e[IDS[e["a"]] != IDS[e["b"]]]
    if region == X.REGION_FROM:
        e = e[e["b"] >= first_new]
    if region == X.REGION_CROSS:
        e = e[(e["a"] < first_new) & (e["b"] >= first_new)]
    assert len(e) and np.array_equal(rows[rows[:, 3] != 0], X.edge_rows(e))
    assert (rows[:, 3] == 0).any() and (rows[:, 2] <= T).all() and (rows[:, 0] < rows[:, 1]).all()


def test_the_definition_by_hand():
    h = np.array([0, 0b1, 1 | 1 << 16 | 1 << 32 | 1 << 48, MASK], np.uint64)
    rows = X.definition(h, threshold=5)
    assert rows.tolist() == [[0, 1, 1, 0b1110], [0, 2, 4, 0], [1, 2, 3, 0b0001]]
    assert X.definition(h, threshold=5, region=X.REGION_FROM, first_new=2).tolist() == [[0, 2, 4, 0], [1, 2, 3, 1]]
    assert X.definition(h, threshold=5, region=X.REGION_CROSS, first_new=1).tolist() == [[0, 1, 1, 0b1110], [0, 2, 4, 0]]
    assert X.definition(h, ids=[5, 5, 6, 7], threshold=5).tolist() == [[0, 2, 4, 0], [1, 2, 3, 1]]
    assert X.definition(h, sizes=[100, 0, 30, 100], size_ratio=0.5, threshold=5).tolist() == [[0, 1, 1, 0b1110], [1, 2, 3, 1]]
    assert len(X.definition(h, threshold=64)) == 6


# ---- the scanner ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [None, 0.5])
def test_candidate_edges_under_exact_are_the_definitions(ctx, ratio):
    files = _files(sizes=SIZES)
    scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, size_ratio=ratio, exact=True))
    got = scanner.candidate_edges(files)
    rows = X.definition(H, ids=UNIQUE, sizes=SIZES, threshold=T, size_ratio=ratio or 0.0)
    assert {k: e.hamming for k, e in got.items()} == _want_edges(rows, UNIQUE)
    assert ctx.exact_calls == 1 and len(ctx.calls) == 1
    banded = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, size_ratio=ratio)).candidate_edges(files)
    assert set(banded) < set(got) and ctx.exact_calls == 1
    assert set(banded) == set(_want_edges(rows[rows[:, 3] != 0], UNIQUE))


def test_the_reference_positional_constructor_still_works():
    cfg = DuplicateScanConfig(6, 0.5, 16, 4, 0.9)
    assert cfg.exact is False and cfg.cosine_threshold == 0.9
    assert [f.name for f in dataclasses.fields(DuplicateScanConfig)][-1] == "exact"


def test_last_counters_count_pairs(ctx):
    files = _files(ids=IDS, sizes=SIZES)
    scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, exact=True))
    edges = scanner.candidate_edges(files)
    rows = X.definition(H, ids=IDS, threshold=T)
    differing = sum(1 for a in range(N) for b in range(a + 1, N) if IDS[a] != IDS[b])
    c = scanner.last_counters
    assert c == {"pairs_evaluated": N * (N - 1) // 2, "pair_total": differing, "after_size": differing, "after_ham": len(rows),
                 "after_cosine": len(rows), "edges": len(edges)}
    # from first_new: the region's pairs; with a size ratio nothing counts the pairs after the size filter alone
    scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, size_ratio=0.5, exact=True))
    scanner.candidate_edges(files, first_new=100)
    rows = X.definition(H, ids=IDS, sizes=SIZES, threshold=T, size_ratio=0.5, region=X.REGION_FROM, first_new=100)
    differing = sum(1 for a in range(N) for b in range(max(a + 1, 100), N) if IDS[a] != IDS[b])
    c = scanner.last_counters
    assert c["pair_total"] == differing and c["after_size"] is None and c["after_ham"] == len(rows) == c["after_cosine"]
    assert c["pairs_evaluated"] == X.region_pairs(N, X.REGION_FROM, 100)


def test_the_funnel_line_prints_na_for_the_size_stage(ctx, caplog):
    scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, size_ratio=0.5, exact=True))
    with caplog.at_level(logging.INFO, logger="dup.scanner"):
        scanner.candidate_edges(_files(sizes=SIZES))
    lines = [r.getMessage() for r in caplog.records]
    assert any("size=n/a" in line for line in lines) and not any("buckets=" in line for line in lines)


def test_with_an_id_twice_the_smallest_a_b_is_kept(ctx):
    """Files 1 and 3 carry one id; file 0 lies 5 bits from file 3 in one band (bands != 0) and 4 bits from file 1 with one in
    every band (bands 0).  The banded order would rank (0, 3) by its bucket; under exact the pair (0, 1) comes first."""
    base = int(H[0])
    hashes = np.array([base, base ^ (1 | 1 << 16 | 1 << 32 | 1 << 48), int(H[1]), base ^ 0b11111], np.uint64)
    files = _files(hashes, ids=np.array([50, 70, 60, 70]))
    got = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, exact=True)).candidate_edges(files)
    assert {k: e.hamming for k, e in got.items()} == {(50, 70): 4}
    banded = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T)).candidate_edges(files)
    assert {k: e.hamming for k, e in banded.items()} == {(50, 70): 5}


def test_a_pair_cap_is_refused_by_the_call_and_ignored_by_the_scanner(ctx, monkeypatch, caplog):
    with pytest.raises(ValueError, match="bucket_pair_cap"):
        _native.Context.hamming_scan(object(), np.zeros(4, np.uint64), 4, exact=True, bucket_pair_cap=10)
    monkeypatch.setenv("KE_DUP_BUCKET_PAIR_CAP", "1")
    scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, exact=True))
    with caplog.at_level(logging.INFO, logger="dup.scanner"):
        got = scanner.candidate_edges(_files())
        scanner.candidate_edges(_files())
    assert set(got) == set(_want_edges(X.definition(H, threshold=T), UNIQUE))
    assert sum("KE_DUP_BUCKET_PAIR_CAP" in r.getMessage() and "ignored" in r.getMessage() for r in caplog.records) == 1


def test_extend_clusters_under_exact_equals_build_clusters_of_the_joined_list(ctx):
    files = _files()
    cfg = DuplicateScanConfig(hamming_threshold=T, exact=True)
    for first_new in (1, 100, N - 1):
        old, new = files[:first_new], files[first_new:]
        previous = DuplicateScanner(cfg).build_clusters(old)
        whole = DuplicateScanner(cfg).build_clusters(files)
        extended = DuplicateScanner(cfg).extend_clusters(old, new, previous)
        assert whole and _same_clusters(extended, whole), first_new
    assert _same_clusters(whole, _clusters_of(files, X.definition(H, threshold=T), UNIQUE))


# ---- the api ---------------------------------------------------------------------------------------------------------------
def test_find_duplicates_and_find_new_duplicates(ctx):
    files = _files()
    rows = X.definition(H, threshold=T)
    want = _clusters_of(files, rows, UNIQUE)
    assert _same_clusters(api.find_duplicates(files, hamming_threshold=T, exact=True), want)
    assert len(api.find_duplicates(files, hamming_threshold=T)) and ctx.exact_calls == 1
    old, new = files[:150], files[150:]
    new_ids = {f.file_id for f in new}
    got = api.find_new_duplicates(old, new, hamming_threshold=T, exact=True)
    from_rows = X.definition(H, threshold=T, region=X.REGION_FROM, first_new=150)
    assert _same_clusters(got, [c for c in _clusters_of(files, from_rows, UNIQUE) if any(e.file.file_id in new_ids for e in c.files)])
    previous = api.find_duplicates(old, hamming_threshold=T, exact=True)
    got = api.find_new_duplicates(old, new, previous=previous, hamming_threshold=T, exact=True)
    assert _same_clusters(got, [c for c in want if any(e.file.file_id in new_ids for e in c.files)])


def test_run_duplicate_scan_takes_exact_through_its_config(ctx):
    rows = [{"file_id": int(UNIQUE[i]), "path": f"lib/f{i:04d}.png", "size": 1000 + i, "width": 100, "height": 100, "phash_u64": int(H[i])}
            for i in range(N)]
    got = api.run_duplicate_scan(rows, config=DuplicateScanConfig(hamming_threshold=T, exact=True))
    assert _same_clusters(got, _clusters_of(_files(), X.definition(H, threshold=T), UNIQUE)) and ctx.exact_calls == 1
    assert len(api.run_duplicate_scan(rows, config=DuplicateScanConfig(hamming_threshold=T))) and ctx.exact_calls == 1


def _flip(word, *bits):
    for b in bits:
        word = int(word) ^ (1 << b)
    return np.uint64(word & MASK)


BANDLESS = (3, 19, 35, 51, 60, 61)                    # six bits, one at least in every 16-bit band


def _views():
    """8 files of unrelated stored hashes; turned / cut rows random except the planted band-less views: orientation 3 of file 5
    is file 1's picture, the crop of file 6 is file 2's picture, the crop of file 7 turned by 5 is file 3's picture -- each
    six bits away with a flipped bit in every band."""
    rng = np.random.default_rng(77)
    stored = rng.integers(0, 1 << 64, 8, dtype=np.uint64)
    tn = rng.integers(0, 1 << 64, (8, 8), dtype=np.uint64)
    cut = rng.integers(0, 1 << 64, (8, 8), dtype=np.uint64)
    tn[:, 0] = stored
    tn[5, 3] = _flip(stored[1], *BANDLESS)
    cut[6, 0] = _flip(stored[2], *BANDLESS)
    cut[7, 5] = _flip(stored[3], *BANDLESS)
    files = [DuplicateFile(10 + i, Path(f"lib/f{i}.png"), 1000, 100, 100, int(stored[i])) for i in range(8)]
    boxes = np.array([[1, 2, 30 + i, 40 + i] for i in range(8)], np.int32)
    return files, tn, cut, boxes


@pytest.fixture
def signatures(monkeypatch):
    files, tn, cut, boxes = _views()
    yes = np.ones(8, bool)
    monkeypatch.setattr(turned, "turned_signatures", lambda paths, *, device=0: (tn, yes))
    monkeypatch.setattr(trimmed, "trimmed_signatures", lambda paths, *, tolerance=48, device=0: (cut[:, 0], boxes, yes, yes))
    monkeypatch.setattr(turned_trimmed, "turned_trimmed_signatures", lambda paths, *, tolerance=48, device=0: (tn, cut, boxes, yes, yes))
    return files


def test_the_three_view_searches_find_bandless_views_only_under_exact(ctx, signatures):
    files = signatures
    for call, pair in ((api.find_turned_duplicates, (11, 15)), (api.find_trimmed_duplicates, (12, 16)),
                       (api.find_turned_trimmed_duplicates, (13, 17))):
        clusters, matches = call(files, hamming_threshold=T, exact=True)
        assert [(m.file_id_a, m.file_id_b, m.hamming) for m in matches if (m.file_id_a, m.file_id_b) == pair] == [pair + (6,)], call.__name__
        assert list(pair) in _groups(clusters)
        before = ctx.exact_calls
        clusters, matches = call(files, hamming_threshold=T)
        assert pair not in {(m.file_id_a, m.file_id_b) for m in matches} and list(pair) not in _groups(clusters)
        assert ctx.exact_calls == before
    clusters, matches = api.find_turned_duplicates(files, hamming_threshold=T, exact=True)
    assert matches == [TurnedMatch(11, 15, 3, 6)]


def test_the_turned_view_scan_under_exact_is_the_definitions_cross_region(ctx):
    files, tn, _, _ = _views()
    got = DuplicateScanner(DuplicateScanConfig(hamming_threshold=T, exact=True)).turned_edges(files, tn)
    call = ctx.calls[-1]
    assert call["exact"] and call["cross"] and call["first_new"] == 8 and call["n"] == 8 + 56
    rows = X.definition(call["hashes"], threshold=T, region=X.REGION_CROSS, first_new=8)
    assert len(rows) == len(got) == 1 and rows[0, 3] == 0


# ---- recall ----------------------------------------------------------------------------------------------------------------
def test_recall_every_planted_pair_within_the_threshold_is_linked_only_under_exact(ctx):
    """12 bases far apart, each with a copy k = 1..8 bits away with its first four flips in four different bands (copies with
    fewer than four flips share a band).  exact links all 12 pairs; the default misses exactly those with k >= 4."""
    rng = np.random.default_rng(5)
    bases = rng.integers(0, 1 << 64, 12, dtype=np.uint64)
    spread = [0, 16, 32, 48, 5, 21, 37, 53]
    copies = [_flip(bases[i], *spread[: 1 + i % 8]) for i in range(12)]
    files = [DuplicateFile(100 + i, Path(f"a/{i}.png"), 1000, 10, 10, int(bases[i])) for i in range(12)]
    files += [DuplicateFile(200 + i, Path(f"b/{i}.png"), 900, 10, 10, int(copies[i])) for i in range(12)]
    planted = [[100 + i, 200 + i] for i in range(12)]
    bandless = [[100 + i, 200 + i] for i in range(12) if 1 + i % 8 >= 4]
    assert len(bandless) == 6
    assert _groups(api.find_duplicates(files, hamming_threshold=T, exact=True)) == planted
    default = _groups(api.find_duplicates(files, hamming_threshold=T))
    assert default == [p for p in planted if p not in bandless]


# ---- the CLI and the worker protocol ------------------------------------------------------------------------------------
def _database(path, files):
    conn = sqlite3.connect(path)
    conn.execute("CREATE TABLE files (id INTEGER PRIMARY KEY, path TEXT, size INTEGER, width INTEGER, height INTEGER, is_present INTEGER)")
    conn.execute("CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER, dhash_u64 INTEGER)")
    for f in files:
        conn.execute("INSERT INTO files VALUES (?, ?, ?, ?, ?, 1)", (f.file_id, str(f.path), f.size, f.width, f.height))
        conn.execute("INSERT INTO signatures VALUES (?, ?, 0)", (f.file_id, f.phash - (1 << 64) if f.phash >= 1 << 63 else f.phash))
    conn.commit()
    conn.close()


def test_scan_dups_exact_combines_with_every_mode(ctx, signatures, tmp_path, capsys):
    files = signatures
    db = str(tmp_path / "k.db")
    _database(db, files)
    assert _groups(cli.scan_database(db, exact=True)) == [] and ctx.exact_calls == 1         # the stored hashes are unrelated
    assert [11, 15] in _groups(cli.scan_database(db, turned=True, exact=True))
    assert [12, 16] in _groups(cli.scan_database(db, trimmed=True, exact=True))
    assert [13, 17] in _groups(cli.scan_database(db, turned_trimmed=True, exact=True))
    assert _groups(cli.scan_database(db, turned=True)) == []
    # --added-like: file 14's stored hash becomes a band-less copy of file 10's
    moved = list(files)
    moved[4] = DuplicateFile(14, Path("incoming/f4.png"), 1000, 100, 100, int(_flip(files[0].phash, *BANDLESS)))
    db2 = str(tmp_path / "k2.db")
    _database(db2, moved)
    assert _groups(cli.scan_database(db2, added_like="incoming/%", exact=True)) == [[10, 14]]
    assert _groups(cli.scan_database(db2, added_like="incoming/%")) == []
    before = ctx.exact_calls
    assert cli.main(["scan-dups", "--db", db2, "--exact"]) == 0 and ctx.exact_calls == before + 1
    assert "1 duplicate group(s), 2 file(s)" in capsys.readouterr().out
    assert cli.main(["scan-dups", "--db", db2]) == 0 and ctx.exact_calls == before + 1
    assert "0 duplicate group(s)" in capsys.readouterr().out
    assert cli.main(["scan-dups", "--db", db, "--exact", "--turned"]) == 0
    assert "1 duplicate group(s), 2 file(s)" in capsys.readouterr().out


def test_the_config_survives_the_trip_to_a_worker():
    r, w = os.pipe()
    try:
        cfg = DuplicateScanConfig(hamming_threshold=11, size_ratio=0.5, exact=True)
        ranks.write_message(w, {"op": "scan", "config": cfg})
        back = ranks.read_message(r)["config"]
    finally:
        os.close(r)
        os.close(w)
    assert back == cfg and back.exact is True and DuplicateScanConfig().exact is False
