"""Tables for tests/test_gpu_scan_from.py and its worker: the smallest at which the scan from first_new (ke_hamming_scan_from)
can go wrong.  n = 2 500 is three row blocks of the 1024 x 1024 tiling, the last one partial.  The hashes are uniform random with
planted pairs at distances 0, THRESHOLD and THRESHOLD + 1 around every position a first_new of the list cuts at, around the
edges of 16-column blocks and 256-column chunks, and inside the diagonal tiles; every planted flip stays above bit 15, so a
planted pair shares at least band 0 under both band configs."""
from __future__ import annotations

import numpy as np

N = 2500
THRESHOLD = 8
FIRST_NEW = (0, 1, 16, 17, 1023, 1024, 1025, 2047, 2048, 2499, 2500)
BIG_N, BIG_FIRST_NEW = 60000, 59000
BIG_FIRST_NEW_WIDE = 30000           # the same table with a region wide enough for the auto rule to take the bucket path
SHARD_FIRST_NEW = (1025, 2048)
PARTS = (3, 8)
SMALL_CAPACITY = 4
CLUSTER_SPLIT = 1500                 # library = the first 1 500 files of the cluster table


def _flip(rng, bits: int) -> np.uint64:
    v = 0
    for b in rng.choice(np.arange(16, 64), size=bits, replace=False):
        v |= 1 << int(b)
    return np.uint64(v)


def planted_table(n: int, cuts, seed: int, long_bucket: int = 40):
    """(hashes, planted pairs as (source, target, distance)).  A target is written once and never after it was read."""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    touched: set = set()
    pairs = []
    dists = (THRESHOLD, 0, THRESHOLD, THRESHOLD + 1)

    def plant(src: int, dst: int, d: int) -> None:
        assert dst not in touched and 0 <= src < n and 0 <= dst < n and src != dst
        h[dst] = h[src] ^ _flip(rng, d)
        touched.update((src, dst))
        pairs.append((src, dst, d))

    # positions first_new - 1 / first_new, ascending so that a source is final before it is read
    for k, f in enumerate(sorted(c for c in cuts if 0 < c < n)):
        plant(f - 1, f, dists[k % len(dists)])
    # around every cut and every block / chunk edge: three partners each, one per distance, from unused positions anywhere
    edges = sorted({p for c in cuts for p in (c - 1, c) if 0 <= p < n} |
                   {p for e in (16, 256, 1040, 1280, 2304, 2496) for p in (e - 1, e) if e < n})
    reserved = set(edges) | touched
    pool = [int(p) for p in rng.permutation(n) if int(p) not in reserved]
    for p in edges:
        for d in (0, THRESHOLD, THRESHOLD + 1):
            plant(p, pool.pop(), d)
    # inside the diagonal tiles: neighbours, a wave's last row against the next wave's first, two waves apart
    for src, dst in ((1030, 1031), (1151, 1152), (1100, 1400), (5, 900), (2060, 2490)):
        if src < n and dst < n and src not in touched and dst not in touched:
            plant(src, dst, THRESHOLD)
    # one long bucket of band 0 (16 x 4), members on either side of most cuts: over a pair cap of 100 as a whole
    base = h[pool.pop()]
    for _ in range(long_bucket):
        q = pool.pop()
        h[q] = base ^ _flip(rng, int(rng.integers(0, 5)))
        touched.add(q)
    return h, pairs


def small_cases() -> dict:
    """name -> dict(h, ids, sizes, kw): with and without duplicate ids, the size filter, the pair cap, and both band configs."""
    h, pairs = planted_table(N, FIRST_NEW, 20260113)
    rng = np.random.default_rng(7)
    ids = np.arange(N, dtype=np.int64) + 100
    for src, dst, _ in pairs[::4]:
        ids[dst] = ids[src]                               # every fourth planted pair is one file twice
    sizes = rng.integers(1000, 1100, size=N).astype(np.int64)
    sizes[rng.integers(0, N, size=50)] = 0                # a missing size passes with everyone
    kw = dict(threshold=THRESHOLD, band_bits=16, band_count=4, size_ratio=0.0, bucket_pair_cap=0)
    return {
        "plain": dict(h=h, ids=None, sizes=None, kw=kw),
        "ids": dict(h=h, ids=ids, sizes=None, kw=kw),
        "sizes": dict(h=h, ids=None, sizes=sizes, kw=dict(kw, size_ratio=0.95)),
        "cap": dict(h=h, ids=None, sizes=None, kw=dict(kw, bucket_pair_cap=100)),
        "8x8": dict(h=h, ids=None, sizes=None, kw=dict(kw, band_bits=8, band_count=8)),
        "all-8x8": dict(h=h, ids=ids, sizes=sizes, kw=dict(kw, band_bits=8, band_count=8, size_ratio=0.95, bucket_pair_cap=100)),
    }


def big_case() -> dict:
    h, _ = planted_table(BIG_N, (BIG_FIRST_NEW, 58368, 59392), 99, long_bucket=20)
    return dict(h=h, ids=None, sizes=None, kw=dict(threshold=THRESHOLD, band_bits=16, band_count=4, size_ratio=0.0, bucket_pair_cap=0))


def cluster_files():
    """DuplicateFile fields for the 2 500 table: (file_id, path, size, width, height, phash) per position."""
    h, _ = planted_table(N, FIRST_NEW, 20260113)
    rng = np.random.default_rng(11)
    ext = ("jpg", "png", "webp", "gif")
    return [(1000 + i, f"lib/d{i % 7}/f{i:05d}.{ext[i % 4]}", int(rng.integers(1000, 1040)), int(rng.integers(100, 104)),
             int(rng.integers(100, 104)), int(h[i])) for i in range(N)]


def bucket_ratio_from() -> int:
    """kBucketRatioFrom of csrc/ke_scan.hip: the auto rule's ratio for a scan from first_new."""
    import os
    import re

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kobato-eyes_amd", "csrc", "ke_scan.hip")
    with open(src) as f:
        return int(re.search(r"kBucketRatioFrom = (\d+);", f.read()).group(1))


def region_pairs(n: int, f: int) -> int:
    return n * (n - 1) // 2 - f * (f - 1) // 2
