"""The scan from first_new (ke_hamming_scan_from, csrc/ke_scan.hip: ke_scan_tiles_from and ke_bucket_pairs_from) on the tables
of tests/_scan_from_cases.py.  Every table runs under KE_SCAN_MODE=auto, tiles and buckets, each mode in a fresh child process
(the library reads the mode once), one after the other.  In every mode the sorted (a, b, h, bands) must equal the oracle's
reference-shaped banded scan filtered by b >= first_new, and the existing ke_hamming_scan of the same table filtered the same way;
counters[0] is the region's closed form, [1] and [2] are taken over the emitted edges, [3] stays the whole table's."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _scan_bucket_cases as B
import _scan_from_cases as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("auto", "tiles", "buckets")
CASES = S.small_cases()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """mode -> the arrays its child process wrote.  One child at a time, each under its own time limit; after one that fails,
    ends on a signal or runs into its limit, no further child is started."""
    work = tmp_path_factory.mktemp("scan_from")
    worker = os.path.join(ROOT, "tests", "_scan_from_worker.py")
    got = {}
    for m in MODES:
        res = subprocess.run(["timeout", "-k", "10", "180", sys.executable, worker, ROOT, str(work / f"{m}.npz")],
                             env=dict(os.environ, KE_SCAN_MODE=m), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, f"KE_SCAN_MODE={m}: exit {res.returncode}\n{res.stdout[-3000:]}"
        got[m] = dict(np.load(str(work / f"{m}.npz")))
        assert str(got[m]["mode"]) == m
    return got


def _oracle_rows(c):
    """(sorted edge rows of the whole table, its bucket pairs): positional truth, as tests/fuzz_scan.py takes it -- the oracle
    without ids, pairs of equal id dropped afterwards."""
    kw = c["kw"]
    exp, exp_c = O.scan_banded(c["h"], ids=None, sizes=c["sizes"], **kw)
    if c["ids"] is not None:
        exp = exp[c["ids"][exp["a"]] != c["ids"][exp["b"]]]
    rows = np.stack([exp["a"].astype(np.int64), exp["b"].astype(np.int64), exp["h"].astype(np.int64), exp["bands"].astype(np.int64)],
                    axis=1).reshape(-1, 4)
    return rows[np.lexsort(rows.T[::-1])], int(exp_c[0])


@pytest.fixture(scope="module")
def truth():
    """name -> (sorted edge rows of the whole table, bucket pairs of the whole table) from the oracle, computed once."""
    return {name: _oracle_rows(c) for name, c in CASES.items()}


def _from(rows, f):
    return rows[rows[:, 1] >= f]


def _ham(rows):
    return sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in rows[:, 3])


def test_the_tables_hold_what_they_are_for(truth):
    """Every first_new of the list cuts through planted pairs: some edge lies wholly below it, some straddles it, some lies wholly
    above it (where the cut leaves room), and the pair (first_new - 1, first_new) is planted."""
    rows, _ = truth["plain"]
    have = set(map(tuple, rows[:, :2].tolist()))
    assert sum((f - 1, f) in have for f in S.FIRST_NEW if 0 < f < S.N) >= 6
    for f in S.FIRST_NEW:
        a, b = rows[:, 0], rows[:, 1]
        if f >= 17:
            assert (b < f).any(), f
        if 0 < f < S.N:
            assert ((a < f) & (b >= f)).any(), f
        if f <= 2048:
            assert (a >= f).any(), f
    assert len(truth["ids"][0]) < len(rows) and len(truth["sizes"][0]) < len(rows) and len(truth["cap"][0]) < len(rows)
    h = CASES["plain"]["h"]
    vals, counts = np.unique(h & np.uint64(0xFFFF), return_counts=True)
    long_members = np.nonzero((h & np.uint64(0xFFFF)) == vals[np.argmax(counts)])[0]
    assert counts.max() * (counts.max() - 1) // 2 > 100 and long_members.min() < 1023 and long_members.max() >= 2048


@pytest.mark.parametrize("first_new", S.FIRST_NEW)
@pytest.mark.parametrize("name", list(CASES))
def test_the_region_is_the_full_scan_filtered(runs, truth, name, first_new):
    rows, bucket_pairs = truth[name]
    want = _from(rows, first_new)
    counters = [S.region_pairs(S.N, first_new), _ham(want), len(want), bucket_pairs]
    for m in MODES:
        got = runs[m]
        edges = got[f"{name}/{first_new}/edges"]
        assert np.array_equal(edges, want), (name, first_new, m, "oracle", len(edges), len(want))
        assert np.array_equal(edges, _from(got[f"{name}/full/edges"], first_new)), (name, first_new, m, "ke_hamming_scan")
        assert got[f"{name}/{first_new}/counters"].tolist() == counters, (name, first_new, m)
        assert int(got[f"{name}/{first_new}/counters"][3]) == int(got[f"{name}/full/counters"][3])
    assert runs["tiles"][f"{name}/{first_new}/path"] == 0
    assert runs["buckets"][f"{name}/{first_new}/path"] == 1


def test_nothing_new_gives_nothing(runs):
    for m in MODES:
        for name in CASES:
            assert len(runs[m][f"{name}/{S.N}/edges"]) == 0
            assert runs[m][f"{name}/{S.N}/counters"][:3].tolist() == [0, 0, 0]


def test_first_new_outside_the_table_is_refused(runs):
    for m in MODES:
        assert runs[m]["einval"].tolist() == [-1, -1]      # KE_EINVAL


@pytest.mark.parametrize("parts", S.PARTS)
@pytest.mark.parametrize("first_new", S.SHARD_FIRST_NEW)
def test_shards_partition_the_region(runs, truth, first_new, parts):
    rows, bucket_pairs = truth["plain"]
    want = _from(rows, first_new)
    for m in MODES:
        got = runs[m]
        edges = got[f"shards/{first_new}/{parts}/edges"]
        assert len(edges) == len(want), (m, "an edge is missing or appears twice")
        assert np.array_equal(edges[np.lexsort(edges.T[::-1])], want), m
        cnt = got[f"shards/{first_new}/{parts}/counters"]
        assert int(cnt[:, 0].sum()) == S.region_pairs(S.N, first_new), m
        assert int(cnt[:, 1].sum()) == _ham(want) and int(cnt[:, 2].sum()) == len(want), m
        assert cnt[:, 3].tolist() == [bucket_pairs] * parts, m
        assert len(set(got[f"shards/{first_new}/{parts}/paths"].tolist())) == 1, (m, "every shard must take the same path")


def test_a_small_edge_buffer_reports_the_whole_count(runs, truth):
    want = _from(truth["plain"][0], 1025)
    assert len(want) > S.SMALL_CAPACITY
    have = set(map(tuple, want.tolist()))
    for m in MODES:
        assert runs[m]["small-capacity/reported"].tolist() == [len(want), len(want)], m
        stored = runs[m]["small-capacity/stored"]
        assert len(stored) == S.SMALL_CAPACITY and set(map(tuple, stored.tolist())) <= have, m


@pytest.mark.parametrize("tag, first_new, auto_path", [("from", S.BIG_FIRST_NEW, 0), ("wide", S.BIG_FIRST_NEW_WIDE, 1)])
def test_the_auto_rule_counts_the_region_at_60000(runs, tag, first_new, auto_path):
    """n = 60 000 is above the bucket path's minimum size.  The table's bucket pairs are held against the region's pairs over
    the region's ratio (kBucketRatioFrom), not the whole triangle's: the thin region of 1 000 new files goes to the tile kernel,
    the same table from 30 000 to the bucket kernels.  The path is read from the word the device wrote."""
    big = S.big_case()
    rows, bucket_pairs = _oracle_rows(big)
    want = _from(rows, first_new)
    assert len(want) > 0 and len(want) < len(rows)
    h = big["h"]
    longest = max(int(np.unique((h >> np.uint64(16 * b)) & np.uint64(0xFFFF), return_counts=True)[1].max()) for b in range(4))
    region = S.region_pairs(S.BIG_N, first_new)
    rule = 1 if (S.BIG_N >= B.BUCKET_MIN_N and bucket_pairs <= region // S.bucket_ratio_from() and longest <= B.BUCKET_LONGEST) else 0
    assert rule == auto_path, "the table no longer sits where this case wants it"
    for m in MODES:
        got = runs[m]
        assert np.array_equal(got[f"big/{tag}/edges"], want), (m, "oracle")
        assert np.array_equal(got[f"big/{tag}/edges"], _from(got["big/full/edges"], first_new)), (m, "ke_hamming_scan")
        assert got[f"big/{tag}/counters"].tolist() == [region, _ham(want), len(want), bucket_pairs], m
    assert runs["auto"][f"big/{tag}/path"] == rule
    assert runs["tiles"][f"big/{tag}/path"] == 0 and runs["buckets"][f"big/{tag}/path"] == 1


def test_extend_clusters_equals_build_clusters_of_the_whole(runs):
    for m in MODES:
        clusters = json.loads(str(runs[m]["clusters"]))
        assert clusters["extended"] == clusters["whole"], m
        assert len(clusters["whole"]) > len(clusters["previous"]) > 0
        assert clusters["whole"] != clusters["previous"]
