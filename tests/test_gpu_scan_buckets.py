"""The scan's two paths (csrc/ke_scan.hip: the all-pairs tile kernel and the band-bucket kernels) on the smallest tables
at which each part of the bucket path can go wrong (tests/_scan_bucket_cases.py).  Every case runs under
KE_SCAN_MODE=auto, tiles and buckets, each mode in a fresh child process (the library reads the mode once); all three must
give the same sorted edges (a, b, h, bands) and the same counters[0..3], and those of the oracle's reference-shaped banded
scan (oracle.scan_banded)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import _scan_bucket_cases as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("auto", "tiles", "buckets")
CASES = S.cases()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """mode -> the arrays its child process wrote.  One child at a time; after one that fails, ends on a signal or runs
    into its time limit, no further child is started."""
    work = tmp_path_factory.mktemp("scan_buckets")
    worker = os.path.join(ROOT, "tests", "_scan_bucket_worker.py")
    got = {}
    for m in MODES:
        res = subprocess.run([sys.executable, worker, ROOT, str(work / f"{m}.npz")], env=dict(os.environ, KE_SCAN_MODE=m),
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
        assert res.returncode == 0, f"KE_SCAN_MODE={m}: exit {res.returncode}\n{res.stdout[-3000:]}"
        got[m] = dict(np.load(str(work / f"{m}.npz")))
        assert str(got[m]["mode"]) == m
    return got


@pytest.fixture(scope="module")
def truth():
    """name -> (sorted edge rows, counters[0..3]) from the oracle, computed once."""
    out = {}
    for name, c in CASES.items():
        h, kw, n = c["h"], c["kw"], len(c["h"])
        # positional truth, as tests/fuzz_scan.py takes it: the oracle without ids, pairs of equal id dropped afterwards
        exp, exp_c = O.scan_banded(h, ids=None, sizes=c["sizes"], **kw)
        if c["ids"] is not None:
            exp = exp[c["ids"][exp["a"]] != c["ids"][exp["b"]]]
        d = h[exp["a"]] ^ h[exp["b"]]
        mask = np.uint64((1 << kw["band_bits"]) - 1)
        equal = [((d >> np.uint64(b * kw["band_bits"])) & mask) == 0 for b in range(kw["band_count"])]
        if kw["bucket_pair_cap"] == 0:
            # the mask by the header's rule (bands >= 31 share bit 31), which the oracle's int32 cannot hold for them
            word = np.zeros(len(d), np.uint32)
            for b, eq in enumerate(equal):
                word |= eq.astype(np.uint32) << np.uint32(min(b, 31))
            bands = word.view(np.int32).astype(np.int64)
            assert kw["band_count"] > 31 or np.array_equal(bands, exp["bands"])
        else:
            bands = exp["bands"].astype(np.int64)
        rows = np.stack([exp["a"].astype(np.int64), exp["b"].astype(np.int64), exp["h"].astype(np.int64), bands], axis=1).reshape(-1, 4)
        rows = rows[np.lexsort(rows.T[::-1])]
        ham = int(exp_c[2]) if c["ids"] is None else sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in bands)
        out[name] = (rows, [n * (n - 1) // 2, ham, len(exp), int(exp_c[0])])
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_three_modes_agree_with_each_other_and_the_oracle(runs, truth, name):
    rows, counters = truth[name]
    for m in MODES:
        got = runs[m]
        assert np.array_equal(got[f"{name}/1/edges"], rows), (name, m, len(got[f"{name}/1/edges"]), len(rows))
        assert got[f"{name}/1/counters"][0].tolist() == counters, (name, m)


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c["auto_path"] is not None])
def test_auto_takes_the_path_the_rule_names(runs, name):
    """Read from the path word the device wrote (ke_last_scan_path), not from timing.  Forced modes take their own path
    wherever the bucket path is built (band table of at most 2^18 bins)."""
    c = CASES[name]
    if name.startswith("min-n"):
        assert len(c["h"]) == S.BUCKET_MIN_N - (1 if name == "min-n-minus-1" else 0)
    built = c["kw"]["band_bits"] <= 24 and (c["kw"]["band_count"] << c["kw"]["band_bits"]) <= 1 << 18
    assert runs["auto"][f"{name}/1/paths"].tolist() == [c["auto_path"]]
    assert runs["tiles"][f"{name}/1/paths"].tolist() == [0]
    assert runs["buckets"][f"{name}/1/paths"].tolist() == [1 if built else 0]


def test_the_group_cases_sit_on_either_side_of_the_rule(truth):
    """The longest bucket of the two group tables is exactly L and L + 1 (no chance neighbour), both have at least the minimum
    size, and both pass the ratio test: only the bucket length differs."""
    for name, longest in (("group-of-L", S.BUCKET_LONGEST), ("group-of-L-plus-1", S.BUCKET_LONGEST + 1)):
        h = CASES[name]["h"]
        n = len(h)
        assert max(int(np.unique((h >> np.uint64(16 * b)) & np.uint64(0xFFFF), return_counts=True)[1].max()) for b in range(4)) == longest
        assert n >= S.BUCKET_MIN_N and truth[name][1][3] <= n * (n - 1) // 2 // S.BUCKET_RATIO


@pytest.mark.parametrize("parts", [3, 8])
def test_shards_partition_the_result(runs, truth, parts):
    rows, counters = truth["planted-3000"]
    for m in MODES:
        got = runs[m]
        edges = got[f"planted-3000/{parts}/edges"]
        assert len(edges) == len(rows), (m, "an edge is missing or appears twice")
        assert np.array_equal(edges[np.lexsort(edges.T[::-1])], rows), m
        cnt = got[f"planted-3000/{parts}/counters"]
        assert int(cnt[:, 0].sum()) == counters[0] and int(cnt[:, 1].sum()) == counters[1] and int(cnt[:, 2].sum()) == counters[2], m
        assert cnt[:, 3].tolist() == [counters[3]] * parts, m
        assert len(set(got[f"planted-3000/{parts}/paths"].tolist())) == 1, (m, "every shard must take the same path")


def test_a_small_edge_buffer_reports_the_whole_count(runs, truth):
    rows, counters = truth["small-capacity"]
    cap = CASES["small-capacity"]["capacity"]
    assert len(rows) > cap
    have = set(map(tuple, rows.tolist()))
    for m in MODES:
        assert runs[m]["small-capacity/reported"].tolist() == [len(rows), len(rows)], m
        stored = runs[m]["small-capacity/stored"]
        assert len(stored) == cap and set(map(tuple, stored.tolist())) <= have, m
