"""The exact scan (ke_hamming_scan_exact: the tile kernels of csrc/ke_scan.hip with ScanArgs.exact set, launched in slices)
against the NumPy definition of tests/_scan_exact_cases.py, edge for edge (a, b, h, bands), on the tables built there: bases and
copies with 0..14 flipped bits, at least a third of the pairs within 8 bits with a flipped bit in every 16-bit band.

The sizes are the tiling's edges: 15/16/17 the 16-hash operand tile, 1023/1024/1025 the 1024 x 1024 tile, 2049 a third row block
of one hash, 3000 a ragged 3 x 3 triangle; first_new at 0, 1, inside a tile, on a tile's edge, n - 1 and n.  Slices are forced in a
child process (KE_SCAN_TILES_PER_LAUNCH is read once per process) at n = 5 000, 15 tiles."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _scan_exact_cases as X
from kobato_eyes_amd import _native, api
from kobato_eyes_amd.scanner import DuplicateEdge, DuplicateFile, assemble_clusters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES_N = (0, 1, 2, 15, 16, 17, 1023, 1024, 1025, 2049, 3000)
THRESHOLDS = (0, 3, 8, 12)
KE_EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    return _native.get_context(0)


def _raw(ctx, h, ids, sizes, first_new, region, part, parts, threshold, ratio, capacity, band_bits=16, band_count=4):
    """One ke_hamming_scan_exact call with a buffer of ``capacity`` edges: (rc, reported edge count, the stored edges, counters)."""
    n = len(h)
    buf = np.zeros(max(capacity, 1), _native.EDGE_DTYPE)
    n_edges, cnt = C.c_int64(-1), np.full(4, 99, np.uint64)
    addr = lambda a: None if a is None or len(a) == 0 else a.ctypes.data
    rc = ctx._lib.ke_hamming_scan_exact(ctx._h, addr(h), addr(ids), addr(sizes), n, first_new, region, part, parts, threshold, band_bits,
                                        band_count, float(ratio), buf.ctypes.data if capacity else None, capacity, C.byref(n_edges),
                                        cnt.ctypes.data)
    return rc, int(n_edges.value), buf[: max(0, min(capacity, n_edges.value))], cnt


def _scan(ctx, h, ids, sizes, first_new, region, part, parts, threshold, ratio):
    """The capacity protocol around _raw: (sorted rows, counters)."""
    capacity = 4096
    while True:
        rc, found, stored, cnt = _raw(ctx, h, ids, sizes, first_new, region, part, parts, threshold, ratio, capacity)
        assert rc == 0, _native_error(ctx)
        if found <= capacity:
            return X.edge_rows(stored), cnt
        capacity = found


def _native_error(ctx):
    return ctx._lib.ke_last_error(ctx._h)


def _regions(n):
    out = [(X.REGION_ALL, 0)]
    for f in sorted({f for f in (0, 1, 1000, 1024, n - 1, n) if 0 <= f <= n}):
        out += [(X.REGION_FROM, f), (X.REGION_CROSS, f)]
    return out


@pytest.mark.parametrize("n", SIZES_N)
def test_every_edge_is_the_definitions(ctx, n):
    h, ids, sizes = X.table(n, seed=n)
    checked = edges_seen = bandless_seen = 0
    for threshold in THRESHOLDS + ((64,) if n <= 600 else ()):
        for with_ids, ratio in ((False, 0.0), (True, 0.5)):
            use_ids, use_sizes = (ids, sizes) if with_ids else (None, None)
            everywhere = X.definition(h, ids=use_ids, sizes=use_sizes, threshold=threshold, size_ratio=ratio)     # once, shared
            for region, first_new in _regions(n):
                want = X.in_region(everywhere, region, first_new)
                got, cnt = _scan(ctx, h, use_ids, use_sizes, first_new, region, 0, 1, threshold, ratio)
                where = (n, threshold, region, first_new, with_ids)
                assert np.array_equal(got, want), where
                shared = sum(bin(int(b)).count("1") for b in want[:, 3])
                pairs = X.region_pairs(n, region, first_new) if n >= 2 else 0
                assert cnt.tolist() == [pairs, shared, len(want), 0], where
                if n >= 2:
                    assert ctx.last_scan_path() == 0, where
                if with_ids:                                  # three shards: disjoint, and their union whole
                    parts = [_scan(ctx, h, use_ids, use_sizes, first_new, region, p, 3, threshold, ratio) for p in range(3)]
                    assert np.array_equal(X.sort_rows(np.concatenate([r for r, _ in parts])), want), where
                    assert sum(int(c[0]) for _, c in parts) == pairs and sum(int(c[2]) for _, c in parts) == len(want), where
                checked += 1
                edges_seen += len(want)
                bandless_seen += int((want[:, 3] == 0).sum())
    print(n, "calls held to the definition:", checked, "edges:", edges_seen, "band-less:", bandless_seen)
    if n >= 15:
        assert edges_seen and bandless_seen


@pytest.mark.parametrize("n", [17, 1025, 3000])
def test_a_buffer_below_the_edge_count_reports_the_count_and_the_retry_is_whole(ctx, n):
    h, ids, sizes = X.table(n, seed=n)
    for region, first_new in ((X.REGION_ALL, 0), (X.REGION_FROM, n // 3), (X.REGION_CROSS, n // 3)):
        want = X.definition(h, ids=ids, sizes=sizes, threshold=12, size_ratio=0.5, region=region, first_new=first_new)
        assert len(want) >= 4
        capacity = len(want) // 2
        rc, found, stored, cnt = _raw(ctx, h, ids, sizes, first_new, region, 0, 1, 12, 0.5, capacity)
        assert rc == 0 and found == len(want) == int(cnt[2]) and len(stored) == capacity
        held = {tuple(r) for r in want.tolist()}
        kept = [tuple(r) for r in X.edge_rows(stored).tolist()]
        assert len(set(kept)) == capacity and set(kept) <= held
        rc, found, stored, _ = _raw(ctx, h, ids, sizes, first_new, region, 0, 1, 12, 0.5, found)
        assert rc == 0 and np.array_equal(X.edge_rows(stored), want)
        rc, found, stored, _ = _raw(ctx, h, ids, sizes, first_new, region, 0, 1, 12, 0.5, 0)          # no buffer at all: the count alone
        assert rc == 0 and found == len(want)


def test_bad_arguments_are_einval(ctx):
    h, ids, sizes = X.table(40)
    good = dict(first_new=0, region=X.REGION_ALL, part=0, parts=1, threshold=8, ratio=0.0, capacity=64)
    for change in (dict(region=3), dict(region=-1), dict(region=X.REGION_ALL, first_new=5), dict(region=X.REGION_FROM, first_new=41),
                   dict(region=X.REGION_CROSS, first_new=-1), dict(threshold=65), dict(threshold=-1), dict(part=1, parts=1), dict(parts=0),
                   dict(band_bits=17), dict(band_count=0)):
        rc, _, _, _ = _raw(ctx, h, None, None, **dict(good, **change))
        assert rc == KE_EINVAL, change
    assert _raw(ctx, h, None, None, **good)[0] == 0
    with pytest.raises(ValueError, match="bucket_pair_cap"):
        ctx.hamming_scan(h, 40, exact=True, bucket_pair_cap=5)


def test_the_three_cross_checks_on_one_table_of_3000(ctx):
    n, first_new, threshold = 3000, 1100, X.THRESHOLD
    h, ids, sizes = X.table(n, seed=3)
    for region in ({}, {"first_new": first_new}, {"first_new": first_new, "cross": True}):
        exact, cnt = ctx.hamming_scan(h, n, ids=ids, sizes=sizes, threshold=threshold, size_ratio=0.5, exact=True, **region)
        exact = X.edge_rows(exact)
        banded, _ = ctx.hamming_scan(h, n, ids=ids, sizes=sizes, threshold=threshold, size_ratio=0.5, **region)
        assert len(banded) and np.array_equal(exact[exact[:, 3] != 0], X.edge_rows(banded)), region
        assert (exact[:, 3] == 0).sum() * 3 >= len(exact), region
        ones, _ = ctx.hamming_scan(h, n, ids=ids, sizes=sizes, threshold=threshold, size_ratio=0.5, band_bits=1, band_count=64, **region)
        assert np.array_equal(exact[:, :3], X.edge_rows(ones)[:, :3]), region
        assert int(cnt[3]) == 0 and int(cnt[2]) == len(exact)
    # every row's neighbours within T are the ranked search's
    exact, _ = ctx.hamming_scan(h, n, threshold=threshold, exact=True)
    exact = X.edge_rows(exact)
    index, distance, count, within = ctx.hamming_nearest(h, h, k=64, max_distance=threshold, ids=np.arange(n), query_ids=np.arange(n))
    assert int(within.max()) <= 64 and int(within.sum()) == 2 * len(exact)
    near = np.array(sorted((q, int(i), int(d)) for q in range(n) for i, d in zip(index[q, : count[q]], distance[q, : count[q]]) if q < i), np.int64)
    assert np.array_equal(near.reshape(-1, 3), exact[:, :3])


@pytest.fixture(scope="module")
def sliced(tmp_path_factory):
    """KE_SCAN_TILES_PER_LAUNCH -> what the child process wrote: '' is one launch.  One child at a time; after one that fails,
    ends on a signal or runs into its time limit, no further child is started."""
    work = tmp_path_factory.mktemp("scan_exact")
    worker = os.path.join(ROOT, "tests", "_scan_exact_worker.py")
    got = {}
    for per in ("", "1", "3"):
        env = {k: v for k, v in os.environ.items() if k != "KE_SCAN_TILES_PER_LAUNCH"}
        if per:
            env["KE_SCAN_TILES_PER_LAUNCH"] = per
        out = str(work / f"per_{per or 'all'}.npz")
        res = subprocess.run([sys.executable, worker, ROOT, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             timeout=180)
        assert res.returncode == 0, f"KE_SCAN_TILES_PER_LAUNCH={per!r}: exit {res.returncode}\n{res.stdout[-3000:]}"
        got[per] = dict(np.load(out))
        assert str(got[per]["per_launch"]) == per
    return got


@pytest.mark.parametrize("name, region, first_new", [("all", X.REGION_ALL, 0), ("from", X.REGION_FROM, 2100), ("cross", X.REGION_CROSS, 2100)])
def test_slices_of_one_and_of_three_tiles_give_what_one_launch_gives(sliced, name, region, first_new):
    n = 5000
    h, ids, sizes = X.table(n, seed=5)
    want = X.definition(h, ids=ids, sizes=sizes, threshold=X.THRESHOLD, size_ratio=0.5, region=region, first_new=first_new)
    assert len(want) > 100 and (want[:, 3] == 0).any()
    for parts in (1, 3):
        one = sliced[""][f"{name}/{parts}/counters"]
        assert int(one[:, 0].sum()) == X.region_pairs(n, region, first_new)
        for per in ("", "1", "3"):
            got = sliced[per]
            assert np.array_equal(X.sort_rows(got[f"{name}/{parts}/edges"]), want), (name, parts, per)
            assert np.array_equal(got[f"{name}/{parts}/counters"], one), (name, parts, per)


def test_find_duplicates_exact_on_written_files(ctx, tmp_path):
    files = []
    for fid, (name, picture) in enumerate(X.pictures()):
        path = tmp_path / name
        picture.save(path, quality=40) if name.endswith(".jpg") else picture.save(path)
        phash = api.compute_signature(str(path))[0] & ((1 << 64) - 1)
        files.append(DuplicateFile(100 + fid, Path(path), os.path.getsize(path), 96, 96, phash))
    h = np.array([f.phash for f in files], np.uint64)
    for threshold in (8, 14):
        rows = X.definition(h, threshold=threshold)
        want = assemble_clusters(files, [DuplicateEdge(100 + int(a), 100 + int(b), int(d)) for a, b, d, _ in rows]) if len(rows) else []
        got = api.find_duplicates(files, hamming_threshold=threshold, exact=True)
        flat = lambda cs: [(c.keeper_id, [(e.file.file_id, e.best_hamming) for e in c.files]) for c in cs]
        print(threshold, "pairs within:", len(rows), "band-less:", int((rows[:, 3] == 0).sum()), "groups:", [[e.file.path.name for e in c.files] for c in got])
        assert flat(got) == flat(want)
        banded = {frozenset((100 + int(a), 100 + int(b))) for a, b, _, bands in rows if bands}
        plain = api.find_duplicates(files, hamming_threshold=threshold)
        linked = {frozenset((x.file.file_id, y.file.file_id)) for c in plain for x in c.files for y in c.files if x is not y}
        assert banded <= linked
    assert len(X.definition(h, threshold=14)) >= 4               # the corpus does hold near-duplicates
