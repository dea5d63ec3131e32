"""extend_clusters and find_new_duplicates without a GPU: the context is replaced by a stand-in whose hamming_scan is the
oracle's reference-shaped banded scan filtered by b >= first_new -- what ke_hamming_scan_from is specified to return -- so what
is held here is the host side: previous clusters standing in for the library's own edges, best_hamming carried over, keepers
and order from the same keys as a scan of the whole table (oracle.assemble_clusters over all edges)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from kobato_eyes_amd import _native, api
from kobato_eyes_amd.scanner import DuplicateFile, DuplicateScanConfig, DuplicateScanner
from oracle import oracle as O

THRESHOLD = 8


class _Context:
    """hamming_scan of _native.Context by the oracle: positional truth, pairs of equal id dropped, then the region's filter."""

    def __init__(self):
        self.calls = []

    def hamming_scan(self, hashes, n, *, ids=None, sizes=None, threshold=8, band_bits=16, band_count=4, size_ratio=0.0,
                     bucket_pair_cap=0, part_index=0, part_count=1, capacity=None, first_new=0):
        self.calls.append(int(first_new))
        if n < 2:
            return np.zeros(0, _native.EDGE_DTYPE), np.zeros(4, np.uint64)
        edges, c = O.scan_banded(hashes, ids=None, sizes=sizes, threshold=threshold, band_bits=band_bits, band_count=band_count,
                                 size_ratio=size_ratio, bucket_pair_cap=bucket_pair_cap)
        if ids is not None:
            edges = edges[ids[edges["a"]] != ids[edges["b"]]]
        edges = edges[edges["b"] >= first_new]
        out = np.zeros(len(edges), _native.EDGE_DTYPE)
        for k in ("a", "b", "h", "bands"):
            out[k] = edges[k]
        ham = sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in out["bands"])
        return out, np.array([n * (n - 1) // 2 - first_new * (first_new - 1) // 2 if first_new else n * (n - 1) // 2, ham, len(out),
                              int(c[0])], np.uint64)


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.delenv("KE_DUP_BUCKET_PAIR_CAP", raising=False)
    c = _Context()
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": c)
    return c


def _file(fid, phash, size=1000, w=100, h=100, ext="jpg", name=None):
    return DuplicateFile(fid, Path(f"lib/d{fid}/{name or f'f{fid:04d}'}.{ext}"), size, w, h, int(phash) & ((1 << 64) - 1))


def _bits(*positions):
    v = 0
    for p in positions:
        v |= 1 << p
    return v


def _flat(clusters):
    return [(c.keeper_id, [(e.file.file_id, e.best_hamming) for e in c.files]) for c in clusters]


def _whole(files):
    """The clusters of the whole table by the oracle alone: its banded scan, then its restatement of the reference's assembly."""
    if len(files) < 2:
        return []
    h = np.array([f.phash for f in files], np.uint64)
    edges, _ = O.scan_banded(h, threshold=THRESHOLD)
    dicts = [dict(file_id=f.file_id, path=f.path.as_posix(), size=f.size, width=f.width, height=f.height) for f in files]
    return O.assemble_clusters(dicts, [(files[a].file_id, files[b].file_id, int(hh)) for a, b, hh in
                                       zip(edges["a"].tolist(), edges["b"].tolist(), edges["h"].tolist())])


def _scanner():
    return DuplicateScanner(DuplicateScanConfig(hamming_threshold=THRESHOLD))


def _extend(library, added):
    s = _scanner()
    previous = s.build_clusters(library)
    assert _flat(previous) == _whole(library)
    return previous, s.extend_clusters(library, added, previous)


def _random_files(rng):
    """Some 40 files around a few base hashes: flips of up to 7 bits above bit 15 (band 0 stays shared), so that families hold
    edges, chains over two edges and pairs past the threshold; few distinct sizes, resolutions and names, so that keys tie."""
    n = int(rng.integers(2, 60))
    bases = rng.integers(0, 1 << 63, size=int(rng.integers(1, 6)), dtype=np.uint64)
    files = []
    for i in rng.permutation(n).tolist():
        flips = _bits(*rng.choice(np.arange(16, 64), size=int(rng.integers(0, 8)), replace=False).tolist())
        files.append(_file(10 + i, int(bases[int(rng.integers(0, len(bases)))]) ^ flips, size=int(rng.choice([0, 900, 1000, 1000, 1100])),
                           w=int(rng.choice([100, 200])), h=100, ext=str(rng.choice(["jpg", "png", "webp", "gif"])),
                           name=f"n{int(rng.integers(0, 12))}"))
    return files


def test_extend_clusters_equals_the_whole_table_over_200_random_splits(ctx):
    rng = np.random.default_rng(20260113)
    grew = 0
    for _ in range(200):
        files = _random_files(rng)
        cut = int(rng.integers(0, len(files) + 1))
        previous, got = _extend(files[:cut], files[cut:])
        want = _whole(files)
        assert _flat(got) == want, (len(files), cut)
        grew += _flat(previous) != want
    assert grew > 100          # the splits are not trivial ones
    assert any(f > 0 for f in ctx.calls)


P = 0x5A5A_0000_0000_1234
Q = P ^ _bits(*range(20, 32))            # 12 bits from P: no edge between the two families


def test_a_new_file_joins_a_cluster(ctx):
    library = [_file(1, P), _file(2, P ^ _bits(20, 21)), _file(3, 0x0123_4567_89AB_CDEF)]
    previous, got = _extend(library, [_file(4, P ^ _bits(40, 41, 42))])
    assert _flat(got) == _whole(library + [_file(4, P ^ _bits(40, 41, 42))])
    assert len(previous) == 1 and len(got) == 1 and sorted(i for i, _ in _flat(got)[0][1]) == [1, 2, 4]
    assert dict(_flat(got)[0][1]) == {1: 2, 2: 2, 4: 3}
    assert ctx.calls[-1] == 3


def test_a_new_file_merges_two_previous_clusters(ctx):
    library = [_file(1, P), _file(2, P ^ _bits(50)), _file(3, Q), _file(4, Q ^ _bits(51, 52))]
    bridge = _file(5, P ^ _bits(*range(20, 26)))      # 6 bits from P and from Q
    previous, got = _extend(library, [bridge])
    assert len(previous) == 2 and len(got) == 1
    assert _flat(got) == _whole(library + [bridge])
    assert dict(_flat(got)[0][1]) == {1: 1, 2: 1, 3: 2, 4: 2, 5: 6}


def test_an_old_members_best_hamming_drops_to_its_new_edge(ctx):
    library = [_file(1, P), _file(2, P ^ _bits(20, 21, 22, 23))]
    twin = _file(3, P)
    previous, got = _extend(library, [twin])
    assert dict(_flat(previous)[0][1]) == {1: 4, 2: 4}
    assert dict(_flat(got)[0][1]) == {1: 0, 2: 4, 3: 0} and _flat(got) == _whole(library + [twin])


def test_a_cluster_of_new_files_only(ctx):
    library = [_file(1, P), _file(2, P ^ _bits(20)), _file(3, 0x0123_4567_89AB_CDEF)]
    added = [_file(4, Q), _file(5, Q ^ _bits(33))]
    previous, got = _extend(library, added)
    assert _flat(got) == _whole(library + added) and len(got) == 2
    assert sorted(sorted(i for i, _ in members) for _, members in _flat(got)) == [[1, 2], [4, 5]]


def test_a_new_file_becomes_the_keeper(ctx):
    library = [_file(1, P, size=1000), _file(2, P ^ _bits(20), size=900)]
    larger = _file(3, P ^ _bits(21), size=5000)
    previous, got = _extend(library, [larger])
    assert previous[0].keeper_id == 1 and got[0].keeper_id == 3 and got[0].files[0].file.file_id == 3
    assert _flat(got) == _whole(library + [larger])


def test_nothing_added(ctx):
    library = [_file(1, P), _file(2, P ^ _bits(20)), _file(3, Q), _file(4, Q ^ _bits(21))]
    before = len(ctx.calls)
    previous, got = _extend(library, [])
    assert _flat(got) == _flat(previous) == _whole(library) and len(got) == 2
    assert len(ctx.calls) == before + 1               # build_clusters scanned; extending by nothing did not


def test_an_empty_library(ctx):
    added = [_file(1, P), _file(2, P ^ _bits(20)), _file(3, Q)]
    got = _scanner().extend_clusters([], added, [])
    assert _flat(got) == _whole(added) and len(got) == 1


def test_a_pair_cap_is_refused(ctx, monkeypatch):
    library = [_file(1, P), _file(2, P ^ _bits(20))]
    previous = _scanner().build_clusters(library)
    monkeypatch.setenv("KE_DUP_BUCKET_PAIR_CAP", "100")
    with pytest.raises(ValueError, match="KE_DUP_BUCKET_PAIR_CAP"):
        _scanner().extend_clusters(library, [_file(3, P)], previous)


def test_a_file_id_twice_is_refused(ctx):
    library = [_file(1, P), _file(2, P ^ _bits(20))]
    previous = _scanner().build_clusters(library)
    with pytest.raises(ValueError, match="file id 2 occurs twice"):
        _scanner().extend_clusters(library, [_file(2, Q)], previous)
    with pytest.raises(ValueError, match="file id 7 occurs twice"):
        _scanner().extend_clusters(library, [_file(7, Q), _file(7, P)], previous)


def test_previous_naming_a_stranger_is_refused(ctx):
    library = [_file(1, P), _file(2, P ^ _bits(20)), _file(3, P ^ _bits(21))]
    previous = _scanner().build_clusters(library)
    with pytest.raises(ValueError, match="file id 3, which is not in library"):
        _scanner().extend_clusters(library[:2], [_file(4, Q)], previous)


def test_find_new_duplicates_returns_exactly_the_clusters_with_an_added_member(ctx):
    rng = np.random.default_rng(5)
    seen_dropped = 0
    for _ in range(40):
        files = _random_files(rng)
        cut = int(rng.integers(1, len(files) + 1))
        library, added = files[:cut], files[cut:]
        previous = api.find_duplicates(library, hamming_threshold=THRESHOLD)
        whole = api.find_duplicates(files, hamming_threshold=THRESHOLD)
        new_ids = {f.file_id for f in added}
        want = [c for c in _flat(whole) if any(i in new_ids for i, _ in c[1])]
        got = api.find_new_duplicates(library, added, previous=previous, hamming_threshold=THRESHOLD)
        assert _flat(got) == want
        seen_dropped += len(want) < len(whole)
        # without previous: the region's edges alone, every cluster still holds an added file
        alone = api.find_new_duplicates(library, added, hamming_threshold=THRESHOLD)
        assert all(any(i in new_ids for i, _ in c[1]) for c in _flat(alone))
        assert {i for c in _flat(alone) for i, _ in c[1]} <= {i for c in want for i, _ in c[1]}
        assert {i for c in _flat(alone) for i, _ in c[1]} >= {i for c in want for i, _ in c[1]} & new_ids
    assert seen_dropped > 5


def test_find_new_duplicates_takes_rows(ctx):
    rows = [dict(file_id=1, path="a/x.jpg", size=10, width=4, height=4, phash_u64=P),
            dict(file_id=2, path="a/y.jpg", size=10, width=4, height=4, phash_u64=P ^ _bits(20)), dict(file_id=3, path="a/z.jpg")]
    got = api.find_new_duplicates(rows[:1], rows[1:], hamming_threshold=THRESHOLD)
    assert _flat(got) == [(1, [(1, 1), (2, 1)])]


def test_scan_dups_added_like_reports_only_groups_with_an_added_file(ctx, tmp_path, capsys):
    import sqlite3

    from kobato_eyes_amd import cli

    db = str(tmp_path / "k.db")
    conn = sqlite3.connect(db)
    conn.execute("CREATE TABLE files (id INTEGER PRIMARY KEY, path TEXT, size INTEGER, width INTEGER, height INTEGER, is_present INTEGER)")
    conn.execute("CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER, dhash_u64 INTEGER)")
    signed = lambda v: v - (1 << 64) if v >> 63 else v
    rows = [(1, "/lib/a.jpg", P), (2, "/lib/b.jpg", P ^ _bits(20)),                 # a pair inside the library
            (3, "/lib/c.jpg", Q), (4, "/lib/incoming/d.jpg", Q ^ _bits(21)),        # a library file and a new one
            (5, "/lib/incoming/e.jpg", 0x0123_4567_89AB_CDEF)]                      # a new file without a partner
    for fid, path, ph in rows:
        conn.execute("INSERT INTO files VALUES (?, ?, 100, 10, 10, 1)", (fid, path))
        conn.execute("INSERT INTO signatures VALUES (?, ?, 0)", (fid, signed(ph)))
    conn.commit()
    conn.close()
    every = cli.scan_database(db, hamming_threshold=THRESHOLD)
    assert sorted(sorted(e.file.file_id for e in c.files) for c in every) == [[1, 2], [3, 4]]
    new = cli.scan_database(db, hamming_threshold=THRESHOLD, added_like="%/incoming/%")
    assert [sorted(e.file.file_id for e in c.files) for c in new] == [[3, 4]]
    assert ctx.calls[-1] == 3                                                        # three library files in front of the added two
    out_csv = str(tmp_path / "out.csv")
    assert cli.main(["scan-dups", "--db", db, "--added-like", "%/incoming/%", "--csv", out_csv]) == 0
    assert "1 duplicate group(s), 2 file(s)" in capsys.readouterr().out
    with open(out_csv) as f:
        assert [line.split(",")[1] for line in f.read().splitlines()[1:]] == ["3", "4"]
