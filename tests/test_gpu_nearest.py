"""ke_hamming_nearest (csrc/ke_nearest.hip) and what is built on it, held to the definition restated in NumPy
(tests/_nearest_cases.py: xor, popcount, the id filter, np.lexsort((position, distance))).  Every comparison is exact equality
of integers: index, distance, count, within and histogram of every call.

The table sizes straddle the wave (64), the workgroup (256) and the walk's segments (n / 4 rounded up to 64): 1, 2, 63, 64, 65,
255, 256, 257, 1 023, 1 025, 4 099; at 4 099, 8 200 and 33 001 a segment has one, two and eight pairs of whole blocks before its
steps.  The cut is placed inside a tie class at every phase (staircase), across every such edge
(ties), on a table of equal hashes, below k (max_distance), and on the excluded entry (ids)."""
from __future__ import annotations

import io

import numpy as np
import pytest

import _nearest_cases as N
from kobato_eyes_amd import _native, api
from kobato_eyes_amd.scanner import DuplicateFile
from oracle import oracle as O

pytestmark = pytest.mark.gpu
NAMES = ("index", "distance", "count", "within", "histogram")


@pytest.fixture(scope="module")
def ctx():
    return _native.get_context(0)


def held(ctx, hashes, queries, k, max_distance, ids=None, query_ids=None, what=()):
    got = ctx.hamming_nearest(hashes, queries, k=k, max_distance=max_distance, ids=ids, query_ids=query_ids, histogram=True)
    want = N.definition(hashes, queries, k, max_distance, ids, query_ids)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, k, max_distance)
        assert np.array_equal(g, w), (name, what, k, max_distance)
    return got


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 8200, 33001])
def test_random_tables(ctx, n):
    for m in (1, 3, 65):
        hashes, queries = N.random_table(n, m)
        for k in (1, 2, 7, 64, 1024):
            for max_distance in (0, 5, 31, 64):
                held(ctx, hashes, queries, k, max_distance, what=(n, m))
        if n >= 4099:                                                       # the id rule in the whole blocks of both passes
            ids = np.arange(n, dtype=np.int64) % 97
            for k in (7, 1024):
                held(ctx, hashes, queries, k, 31, ids, np.arange(m, dtype=np.int64) % 97, what=(n, m, "ids"))


def test_a_table_of_equal_hashes(ctx):
    value = 0x5DEECE66D1234567
    hashes = np.full(4099, value, np.uint64)
    for k in (1, 64, 1024):
        index, distance, count, within, histogram = held(ctx, hashes, np.array([value], np.uint64), k, 64)
        assert index[0].tolist() == list(range(k)) and not distance.any() and count[0] == k and within[0] == 4099
        assert histogram[0, 0] == 4099


def test_a_staircase_puts_the_cut_inside_a_tie_class_at_every_phase(ctx):
    query = 0x0F1E2D3C4B5A6978
    hashes = N.staircase(1300, query)
    assert np.array_equal(N.popcount64(hashes ^ np.uint64(query)), np.arange(1300) % 65)
    assert len(set(hashes.tolist())) > 1300 - 2 * 20                       # only the 0- and 64-bit entries repeat
    for k in range(1, 131):
        index, distance, *_ = held(ctx, hashes, np.array([query], np.uint64), k, 64)
        assert index[0].tolist() == [65 * (j % 20) + j // 20 for j in range(k)]    # 20 entries per distance, in position order


def test_ties_across_the_edges(ctx):
    query, n = 0x1122334455667788, 1030
    hashes = np.array([N.at_distance(query, 40, i) for i in range(n)], np.uint64)
    for i in (0, 63, 64, 255, 256, 257, 1023, 1024, n - 1):
        hashes[i] = N.at_distance(query, 7, i)
    for i in (62, 65, 254, 258, 1022, 1025):
        hashes[i] = N.at_distance(query, 3, i)
    for k in (1, 5, 6, 7, 14, 15, 16):
        index, *_ = held(ctx, hashes, np.array([query], np.uint64), k, 64)
        assert index[0].tolist() == ([62, 65, 254, 258, 1022, 1025, 0, 63, 64, 255, 256, 257, 1023, 1024, n - 1, 1])[:k]


def test_max_distance_below_the_kth_neighbour(ctx):
    query = 0x00FF00FF00FF00FF
    hashes = np.array([N.at_distance(query, 2 + i % 30, i) for i in range(700)], np.uint64)
    index, distance, count, within, _ = held(ctx, hashes, np.array([query, ~np.uint64(query)], np.uint64), 100, 3)
    assert count.tolist() == [48, 0] and within.tolist() == [48, 0]          # 24 entries at 2 bits, 24 at 3
    assert (index[0, 48:] == -1).all() and (distance[0, 48:] == -1).all() and (index[1] == -1).all() and (distance[1] == -1).all()
    held(ctx, np.zeros(0, np.uint64), np.array([query], np.uint64), 5, 64)  # an empty table: every count 0


def test_ids(ctx):
    query, n = 0x7766554433221100, 600
    hashes = np.array([N.at_distance(query, 20, i) for i in range(n)], np.uint64)
    hashes[300] = query                                                     # the nearest one
    for i in (10, 130, 131, 290, 470):
        hashes[i] = N.at_distance(query, 6, i)                              # a tie class the cut lands in
    ids = np.arange(n, dtype=np.int64) + 1000
    queries = np.array([query, query, query], np.uint64)
    query_ids = np.array([1300, 1131, 5], np.int64)                         # the nearest; inside the tie class; nobody
    for k in (1, 3, 4, 6, 7):
        index, *_ = held(ctx, hashes, queries, k, 64, ids, query_ids)
        assert index[0].tolist() == [10, 130, 131, 290, 470, 0, 1][:k]
        assert index[1].tolist() == [300, 10, 130, 290, 470, 0, 1][:k]
        assert index[2].tolist() == [300, 10, 130, 131, 290, 470, 0][:k]
        for one_sided in (dict(ids=ids), dict(query_ids=query_ids)):        # either array alone excludes nothing
            got = ctx.hamming_nearest(hashes, queries, k=k, **one_sided)
            assert all(row.tolist() == [300, 10, 130, 131, 290, 470, 0][:k] for row in got[0])
    ids[:] = 7                                                              # every entry excluded
    index, distance, count, within, _ = held(ctx, hashes, queries[:1], 4, 64, ids, np.array([7], np.int64))
    assert count[0] == 0 and within[0] == 0


def test_distance_64_and_k_beyond_the_table(ctx):
    rng = np.random.default_rng(N.SEED)
    query = 0xA5A5A5A5DEADBEEF
    hashes = rng.integers(0, 2**64, 500, dtype=np.uint64)
    hashes[[0, 77, 499]] = np.uint64(query ^ (2**64 - 1))
    for k in (500, 501, 1024):
        index, distance, count, within, _ = held(ctx, hashes, np.array([query], np.uint64), k, 64)
        assert count[0] == 500 and within[0] == 500 and sorted(index[0, :500].tolist()) == list(range(500))
        assert index[0, 497:500].tolist() == [0, 77, 499] and distance[0, 497:500].tolist() == [64, 64, 64]


def test_more_queries_than_a_grid_dimension_of_65535(ctx):
    hashes, queries = N.random_table(300, 66000)
    held(ctx, hashes, queries, 3, 64)


def test_device_pointers(ctx):
    n, m, k = 1025, 7, 9
    hashes, queries = N.random_table(n, m)
    ids = (np.arange(n, dtype=np.int64) * 7) % 300
    query_ids = np.arange(m, dtype=np.int64) * 11
    want = N.definition(hashes, queries, k, 31, ids, query_ids)
    sizes = [n * 8, n * 8, m * 8, m * 8, m * k * 8, m * k * 4, m * 4, m * 8, m * 65 * 4]
    dev = [ctx.malloc(s) for s in sizes]
    try:
        for d, a in zip(dev, (hashes, ids, queries, query_ids)):
            ctx.memcpy(d, a, a.nbytes)
        got = ctx.hamming_nearest(dev[0], dev[2], k=k, max_distance=31, ids=dev[1], query_ids=dev[3], histogram=True, n=n, m=m)
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(g, w), name
        mixed = ctx.hamming_nearest(hashes, dev[2], k=k, max_distance=31, ids=dev[1], query_ids=query_ids, histogram=True, n=n, m=m)
        for name, g, w in zip(NAMES, mixed, want):
            assert np.array_equal(g, w), name
        with ctx._lock:                                                     # device outputs: the C call itself
            rc = ctx._lib.ke_hamming_nearest(ctx._h, dev[0], dev[1], n, dev[2], dev[3], m, k, 31, dev[4], dev[5], dev[6], dev[7], dev[8])
        assert rc == 0
        back = [np.empty_like(w) for w in want]
        for a, d in zip(back, (dev[4], dev[5], dev[6], dev[7], dev[8])):
            ctx.memcpy(a, d, a.nbytes)
        for name, g, w in zip(NAMES, back, want):
            assert np.array_equal(g, w), name
    finally:
        for d in dev:
            ctx.free(d)


def test_bad_arguments_are_einval_and_the_context_lives_on(ctx):
    hashes, queries = N.random_table(65, 3)
    out = (np.zeros((3, 1024), np.int64), np.zeros((3, 1024), np.int32), np.zeros(3, np.int32))

    def call(n=65, m=3, k=4, max_distance=64, h=hashes, q=queries, outs=out):
        with ctx._lock:
            return ctx._lib.ke_hamming_nearest(ctx._h, None if h is None else h.ctypes.data, None, n, None if q is None else q.ctypes.data,
                                               None, m, k, max_distance, *[None if o is None else o.ctypes.data for o in outs], None, None)

    assert call() == 0
    for bad in (dict(k=0), dict(k=-1), dict(k=1025), dict(max_distance=-1), dict(max_distance=65), dict(n=-1), dict(n=2**31), dict(m=-1),
                dict(h=None), dict(q=None), dict(outs=(None, out[1], out[2])), dict(outs=(out[0], None, out[2])),
                dict(outs=(out[0], out[1], None))):
        assert call(**bad) == -1, bad
        assert ctx._lib.ke_last_error(ctx._h)
    with pytest.raises(ValueError):
        ctx.hamming_nearest(hashes, queries, k=1025)
    assert call(m=0, q=None, outs=(None, None, None)) == 0                  # no queries: nothing is touched
    assert ctx._lib.ke_hamming_nearest(None, None, None, 0, None, None, 0, 1, 64, None, None, None, None, None) == -1
    held(ctx, hashes, queries, 4, 64)
    assert ctx.last_kernel_ms(9) >= 0.0


def test_end_to_end_the_source_of_a_recompressed_picture_comes_first(ctx, tmp_path):
    from PIL import Image

    n, side = 40, 256
    px = ctx.synth_rgb(O.SEED, 0, n, side, side)
    assert np.array_equal(px, O.synth_rgb_batch(0, n, side, side))
    recompressed, queries = [], []
    for i in range(n):
        blob = io.BytesIO()
        Image.fromarray(px[i]).save(blob, "JPEG", quality=70)
        recompressed.append(np.asarray(Image.open(io.BytesIO(blob.getvalue())).convert("RGB")))
        if i % 2:
            path = tmp_path / f"q{i:02d}.jpg"
            path.write_bytes(blob.getvalue())
            queries.append(str(path))
        else:
            queries.append(Image.open(io.BytesIO(blob.getvalue())))
    # the precondition, from the CPU oracle alone: by its hashes every re-encoding lies nearest its own source
    oracle_lib, _ = O.hash_batch(px)
    oracle_q, _ = O.hash_batch(np.stack(recompressed))
    first = N.definition(oracle_lib, oracle_q, 1, 64)[0][:, 0]
    assert first.tolist() == list(range(n)), "the pictures do not tell their sources apart: choose another seed"

    lib_hashes, _ = ctx.hash_uniform(px, n, side, side, 3)
    assert np.array_equal(lib_hashes, oracle_lib)
    library = [DuplicateFile(100 + i, tmp_path / f"src{i:02d}.png", 1000, side, side, int(lib_hashes[i])) for i in range(n)]
    found = api.find_similar(library, queries, k=3)
    q_hashes = np.array([api.compute_signature(q)[0] & (2**64 - 1) for q in queries], np.uint64)
    index, distance, count, *_ = N.definition(lib_hashes, q_hashes, 3, 64)
    assert [[(h.file.file_id, h.distance) for h in row] for row in found] == \
        [[(100 + int(p), int(d)) for p, d in zip(index[q], distance[q])] for q in range(n)]
    assert [row[0].file.file_id for row in found] == [100 + i for i in range(n)]
