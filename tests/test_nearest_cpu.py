"""The host layers of the ranked search without a GPU: DuplicateScanner.nearest, api.find_similar and the CLI's ``similar``
sub-command over a stand-in context whose ``hamming_nearest`` is the definition of ke_hamming_nearest in NumPy -- xor,
popcount, the id filter, ``np.lexsort((position, distance))`` -- so what is held here is what the host does around the call:
which files enter the table, how positions come back as files, what a query's id excludes, where rows are cut."""
from __future__ import annotations

import csv
import sqlite3
from pathlib import Path

import numpy as np
import pytest

import kobato_eyes_amd
from kobato_eyes_amd import _native, api, cli
from kobato_eyes_amd.scanner import DuplicateFile, DuplicateScanConfig, DuplicateScanner, SimilarFile
from oracle import oracle as O

MASK = (1 << 64) - 1


def nearest_definition(hashes, queries, k, max_distance, ids=None, query_ids=None):
    hashes, queries = np.asarray(hashes, np.uint64), np.asarray(queries, np.uint64)
    m = len(queries)
    index = np.full((m, k), -1, np.int64)
    distance = np.full((m, k), -1, np.int32)
    count = np.zeros(m, np.int32)
    within = np.zeros(m, np.int64)
    hist = np.zeros((m, 65), np.uint32)
    for q in range(m):
        x = hashes ^ queries[q]
        d = np.array([bin(int(v)).count("1") for v in x], np.int64)
        keep = d <= max_distance
        if ids is not None and query_ids is not None:
            keep &= np.asarray(ids) != query_ids[q]
        pos = np.nonzero(keep)[0]
        pos = pos[np.lexsort((pos, d[pos]))]
        c = min(k, len(pos))
        index[q, :c], distance[q, :c], count[q], within[q] = pos[:c], d[pos[:c]], c, len(pos)
        hist[q] = np.bincount(d[pos], minlength=65)
    return index, distance, count, within, hist


class _Context:
    """hamming_nearest of _native.Context by the definition; hamming_scan by the oracle's banded scan, for find_duplicates."""

    def __init__(self):
        self.calls = []

    def hamming_nearest(self, hashes, queries, *, k, max_distance=64, ids=None, query_ids=None, histogram=False, n=None, m=None):
        self.calls.append(dict(n=len(hashes), m=len(queries), k=k, max_distance=max_distance))
        out = nearest_definition(hashes, queries, k, max_distance, ids, query_ids)
        return out if histogram else out[:4]

    def hamming_scan(self, hashes, n, *, ids=None, sizes=None, threshold=8, band_bits=16, band_count=4, size_ratio=0.0,
                     bucket_pair_cap=0, part_index=0, part_count=1, capacity=None, first_new=0):
        edges, c = O.scan_banded(hashes, ids=None, sizes=sizes, threshold=threshold, band_bits=band_bits, band_count=band_count,
                                 size_ratio=size_ratio, bucket_pair_cap=bucket_pair_cap)
        out = np.zeros(len(edges), _native.EDGE_DTYPE)
        for key in ("a", "b", "h", "bands"):
            out[key] = edges[key]
        return out, np.array([n * (n - 1) // 2, 0, len(out), int(c[0])], np.uint64)


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.delenv("KE_DUP_BUCKET_PAIR_CAP", raising=False)
    c = _Context()
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": c)
    return c


def _file(fid, phash, name=None):
    return DuplicateFile(fid, Path(f"lib/{name or f'f{fid:04d}'}.jpg"), 1000, 100, 100, None if phash is None else int(phash) & MASK)


def _bits(*positions):
    v = 0
    for p in positions:
        v |= 1 << p
    return v


def _scanner():
    return DuplicateScanner(DuplicateScanConfig())


BASE = 0x0123456789ABCDEF


def test_files_without_a_hash_are_dropped_and_positions_map_back(ctx):
    library = [_file(10, None), _file(11, BASE ^ _bits(1, 2, 3)), _file(12, None), _file(13, BASE ^ _bits(5)), _file(14, BASE),
               _file(15, None), _file(16, BASE ^ _bits(7, 9))]
    (hits,) = _scanner().nearest(library, [_file(-1, BASE)], k=3)
    assert ctx.calls[-1]["n"] == 4
    assert [(h.file.file_id, h.distance) for h in hits] == [(14, 0), (13, 1), (16, 2)]
    assert all(isinstance(h, SimilarFile) and h.file is f for h, f in zip(hits, (library[4], library[3], library[6])))
    (again,) = api.find_similar(library, [_file(-1, BASE)], k=3)
    assert again == hits


def test_a_query_without_a_hash_gets_nothing_and_keeps_its_place(ctx):
    library = [_file(1, BASE), _file(2, BASE ^ _bits(0))]
    out = _scanner().nearest(library, [_file(-1, None), _file(-1, BASE ^ _bits(0)), _file(-1, None)], k=2)
    assert [[h.file.file_id for h in row] for row in out] == [[], [2, 1], []]
    assert ctx.calls[-1]["m"] == 1
    assert _scanner().nearest([], [_file(-1, BASE)], k=2) == [[]]
    assert _scanner().nearest(library, [], k=2) == []
    assert api.find_similar(library, [{"path": "no/hash.jpg"}, {"file_id": 9, "path": "q.jpg", "phash_u64": BASE}], k=1)[0] == []


def test_a_query_from_the_library_does_not_return_itself_but_returns_its_twin(ctx):
    library = [_file(1, BASE), _file(2, BASE ^ _bits(3, 4)), _file(3, BASE), _file(4, BASE ^ _bits(8))]
    (hits,) = _scanner().nearest(library, [library[0]], k=10)
    assert [(h.file.file_id, h.distance) for h in hits] == [(3, 0), (4, 1), (2, 2)]
    (hits,) = _scanner().nearest(library, [library[2]], k=10)
    assert [(h.file.file_id, h.distance) for h in hits] == [(1, 0), (4, 1), (2, 2)]


def test_a_query_without_an_id_excludes_nothing(ctx):
    library = [_file(1, BASE), _file(-1, BASE ^ _bits(1)), _file(3, BASE ^ _bits(2, 3))]
    for query in (_file(-1, BASE), DuplicateFile(None, Path("q.jpg"), None, None, None, BASE), _file(77, BASE)):
        (hits,) = _scanner().nearest(library, [query], k=10)
        assert [h.distance for h in hits] == [0, 1, 2], query.file_id
        assert [h.file for h in hits] == library


def test_rows_are_cut_at_count_and_k_may_exceed_the_library(ctx):
    library = [_file(i, BASE ^ _bits(*range(i))) for i in range(6)]           # file i at distance i
    out = _scanner().nearest(library, [_file(-1, BASE), _file(-1, BASE ^ MASK)], k=50, max_distance=3)
    assert [(h.file.file_id, h.distance) for h in out[0]] == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert out[1] == []
    out = api.find_similar(library, [_file(-1, BASE)], k=1024)
    assert [h.file.file_id for h in out[0]] == [0, 1, 2, 3, 4, 5]
    assert ctx.calls[-1]["k"] == 1024


def test_no_limit_is_passed_on_as_64_and_the_config_is_not_read(ctx):
    library = [_file(1, BASE ^ MASK)]
    scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=0, size_ratio=0.99, band_bits=8, band_count=2))
    (hits,) = scanner.nearest(library, [_file(-1, BASE)], k=1)
    assert ctx.calls[-1]["max_distance"] == 64 and [(h.file.file_id, h.distance) for h in hits] == [(1, 64)]
    api.find_similar(library, [_file(-1, BASE)], k=1, max_distance=None)
    assert ctx.calls[-1]["max_distance"] == 64
    api.find_similar(library, [_file(-1, BASE)], k=1, max_distance=12)
    assert ctx.calls[-1]["max_distance"] == 12


def test_the_pair_no_band_holds_is_found_here_and_not_by_find_duplicates(ctx):
    """8 bits apart, two differing bits in each 16-bit band: the two hashes share no band, so the banded scan never compares
    them at threshold 8; the ranking by distance alone returns the pair."""
    twin = BASE ^ _bits(0, 9, 16, 25, 32, 41, 48, 57)
    assert bin(BASE ^ twin).count("1") == 8 and all(((BASE ^ twin) >> (16 * band)) & 0xFFFF for band in range(4))
    library = [_file(1, BASE), _file(2, twin), _file(3, BASE ^ MASK)]
    assert api.find_duplicates(library, hamming_threshold=8) == []
    (hits,) = api.find_similar(library, [library[0]], k=1)
    assert [(h.file.file_id, h.distance) for h in hits] == [(2, 8)]


def test_find_similar_is_exported_and_hashes_a_picture(ctx, monkeypatch):
    assert kobato_eyes_amd.find_similar is api.find_similar and kobato_eyes_amd.SimilarFile is SimilarFile
    seen = []
    monkeypatch.setattr(api, "compute_signature", lambda item, device=0: (seen.append(item), (-1, 0))[1])      # signed: all ones
    library = [_file(1, MASK ^ _bits(5)), _file(2, 0)]
    out = api.find_similar(library, ["some/picture.png", Path("other.png")], k=1)
    assert seen == ["some/picture.png", Path("other.png")]
    assert [[(h.file.file_id, h.distance) for h in row] for row in out] == [[(1, 1)], [(1, 1)]]


def _database(path, rows):
    conn = sqlite3.connect(path)
    conn.execute("CREATE TABLE files (id INTEGER PRIMARY KEY, path TEXT, size INTEGER, width INTEGER, height INTEGER, is_present INTEGER)")
    conn.execute("CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER, dhash_u64 INTEGER)")
    for fid, name, phash in rows:
        conn.execute("INSERT INTO files VALUES (?, ?, 1000, 100, 100, 1)", (fid, name))
        conn.execute("INSERT INTO signatures VALUES (?, ?, 0)", (fid, phash))
    conn.commit()
    conn.close()


def test_the_cli_ranks_the_files_of_a_database(ctx, tmp_path, capsys):
    db, out = str(tmp_path / "k.db"), str(tmp_path / "similar.csv")
    _database(db, [(1, "/photos/a.jpg", BASE), (2, "/photos/b.jpg", BASE ^ _bits(1, 2)), (3, "/incoming/c.jpg", BASE ^ _bits(1)),
                   (4, "/incoming/d.jpg", BASE), (5, "/elsewhere/e.jpg", BASE)])
    assert cli.main(["similar", "--db", db, "--to-like", "/incoming/%", "--k", "2", "--csv", out]) == 0
    with open(out, newline="") as handle:
        rows = list(csv.reader(handle))
    assert rows[0] == ["query", "rank", "path", "distance"]
    assert rows[1:] == [["/incoming/c.jpg", "1", "/photos/a.jpg", "1"], ["/incoming/c.jpg", "2", "/photos/b.jpg", "1"],
                        ["/incoming/d.jpg", "1", "/photos/a.jpg", "0"], ["/incoming/d.jpg", "2", "/elsewhere/e.jpg", "0"]]
    capsys.readouterr()
    assert cli.main(["similar", "--db", db, "--to-like", "/incoming/d%", "--like", "/%o%/%", "--k", "5", "--max-distance", "1"]) == 0
    printed = list(csv.reader(capsys.readouterr().out.splitlines()))
    assert printed == [["query", "rank", "path", "distance"], ["/incoming/d.jpg", "1", "/photos/a.jpg", "0"],
                       ["/incoming/d.jpg", "2", "/incoming/c.jpg", "1"]]
    with pytest.raises(SystemExit):
        cli.main(["similar", "--db", db])
