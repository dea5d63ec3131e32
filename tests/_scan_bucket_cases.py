"""The tables of tests/test_gpu_scan_buckets.py, built the same way in the test and in its child processes
(tests/_scan_bucket_worker.py): the smallest shapes at which each part of the scan's bucket path can go wrong."""
from __future__ import annotations

import os
import re

import numpy as np

U = np.uint64
# the rule between the two paths, read from where it is stated: the cases below sit on either side of each constant
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kobato-eyes_amd", "csrc", "ke_scan.hip")).read()
BUCKET_RATIO, BUCKET_LONGEST = map(int, re.search(r"kBucketRatio = (\d+), kBucketLongest = (\d+);", _SRC).groups())
BUCKET_MIN_N = int(re.search(r"kBucketMinN = (\d+);", _SRC).group(1))


def _rand(rng, n):
    return rng.integers(0, 2**63, n, dtype=U) * U(2) + rng.integers(0, 2, n, dtype=U)


def _flip(x, bits):
    for b in bits:
        x ^= 1 << int(b)
    return x


def planted(n, seed):
    """Random hashes; about a third are copies of an earlier one with 0..10 flipped bits."""
    rng = np.random.default_rng(seed)
    h = _rand(rng, n)
    for i in range(1, n):
        if i == 1 or rng.integers(0, 3) == 0:
            src = int(rng.integers(0, i))
            h[i] = U(_flip(int(h[src]), rng.choice(64, int(rng.integers(0, 11)), replace=False)))
    return h


def shared_bands(seed):
    """Pairs that share exactly 1, 2, 3 and 4 of the 16 x 4 bands (one flipped bit in each band they do not share), every
    subset of bands, among random filler."""
    rng = np.random.default_rng(seed)
    out = list(_rand(rng, 40))
    for mask in range(1, 16):                                   # bit b set: band b is shared
        x = int(_rand(rng, 1)[0])
        out += [U(x), U(_flip(x, [16 * b + int(rng.integers(0, 16)) for b in range(4) if not mask >> b & 1]))]
    return np.array(out, dtype=U)[rng.permutation(len(out))]


def high_bands(seed):
    """2 x 32 bands: pairs whose only shared bands are 30, 31, both, and 29 + 31 (one flipped bit in every other band), among
    random filler whose pairs share many bands by chance."""
    rng = np.random.default_rng(seed)
    out = list(_rand(rng, 90))
    for keep in ([30], [31], [30, 31], [29, 31], [0, 31]):
        x = int(_rand(rng, 1)[0])
        out += [U(x), U(_flip(x, [2 * b + int(rng.integers(0, 2)) for b in range(32) if b not in keep]))]
    return np.array(out, dtype=U)[rng.permutation(len(out))]


def one_group(group, seed, n):
    """n random hashes and `group` copies of one more; no random hash shares a band value with the group, so the group's
    four buckets hold exactly `group` members and every other bucket is a chance bucket of a few."""
    rng = np.random.default_rng(seed)
    g = int(_rand(rng, 1)[0])
    fill = _rand(rng, n)
    for b in range(4):
        same = (fill >> U(16 * b)) & U(0xFFFF) == U((g >> (16 * b)) & 0xFFFF)
        fill[same] ^= U(1 << (16 * b))
    h = np.concatenate([fill, np.full(group, g, dtype=U)])
    return h[rng.permutation(len(h))]


def group_table_size(group):
    """Filler size at which a group of that length still passes the ratio test with room for the chance buckets:
    4 C(group, 2) + 4 n^2 / (2 * 65536) <= (n^2 / 2) / BUCKET_RATIO / 2, and at least BUCKET_MIN_N."""
    need = 4 * group * (group - 1) // 2
    n = BUCKET_MIN_N
    while 2 * (need + 4 * n * n // (2 * 65536)) > n * (n - 1) // 2 // BUCKET_RATIO:
        n += 8192
    return n


def capped(seed):
    """Band 0 holds a bucket of 3 and a bucket of 6 (pair cap 5 lies between C(3,2) = 3 and C(6,2) = 15).  Members of the
    large bucket are near-duplicates; two of them also share band 1, so that pair must appear with band 1 alone."""
    rng = np.random.default_rng(seed)
    out = [U(int(v) & ~0xFFFF | int(rng.integers(2, 0x10000))) for v in _rand(rng, 150)]   # filler: other band-0 values
    small, large = int(_rand(rng, 1)[0]) & ~0xFFFF, int(_rand(rng, 1)[0]) & ~0xFFFF | 1
    for k in range(3):
        out.append(U(_flip(small, [16 + k])))                    # share bands 0, 2, 3
    for k in range(4):
        out.append(U(_flip(large, [16 + k, 32 + k, 48 + k])))   # share band 0 only ...
    for k in (8, 9):
        out.append(U(_flip(large, [32 + k, 48 + k])))           # ... but these two share band 1 as well
    return np.array(out, dtype=U)[rng.permutation(len(out))]


def cases():
    """name -> dict(h, ids, sizes, kw (scan parameters), parts, capacity, auto_path)."""
    c = {}

    def add(name, h, ids=None, sizes=None, parts=(1,), capacity=None, auto_path=None, **kw):
        kw = dict(dict(threshold=8, band_bits=16, band_count=4, size_ratio=0.0, bucket_pair_cap=0), **kw)
        c[name] = dict(h=h, ids=ids, sizes=sizes, kw=kw, parts=tuple(parts), capacity=capacity, auto_path=auto_path)

    for n in (2, 17, 1025, 3000):
        add(f"planted-{n}", planted(n, 100 + n), parts=(1, 3, 8) if n == 3000 else (1,))
    add("shared-bands", shared_bands(7))
    add("bands-30-31", high_bands(8), threshold=40, band_bits=2, band_count=32)
    n = group_table_size(BUCKET_LONGEST + 1)
    add("group-of-L", one_group(BUCKET_LONGEST, 9, n), auto_path=1)              # longest bucket == L: buckets
    add("group-of-L-plus-1", one_group(BUCKET_LONGEST + 1, 10, n), auto_path=0)  # one more: tiles
    add("min-n-minus-1", _rand(np.random.default_rng(18), BUCKET_MIN_N - 1), auto_path=0)   # n >= kBucketMinN, at the border
    add("min-n", _rand(np.random.default_rng(18), BUCKET_MIN_N), auto_path=1)
    add("skew-long-group", one_group(300, 10, 2000), auto_path=0)                # small and skewed: tiles
    rng = np.random.default_rng(11)
    add("one-bit-bands", _rand(rng, 500), threshold=20, band_bits=1, band_count=64, auto_path=0)
    add("pair-cap", capped(12), bucket_pair_cap=5)
    n = 1500
    h = planted(n, 13)
    add("ids-sizes", h, ids=rng.integers(0, n // 2, n).astype(np.int64), sizes=rng.integers(0, 5000, n).astype(np.int64), size_ratio=0.5)
    add("sizes-0.9", h, sizes=rng.integers(0, 5000, n).astype(np.int64), size_ratio=0.9, bucket_pair_cap=50)
    add("no-sizes-with-ratio", h, sizes=None, size_ratio=0.9)
    add("threshold-0", planted(600, 14), threshold=0)
    add("threshold-64", planted(300, 15), threshold=64)
    add("small-capacity", planted(1025, 16), capacity=8)
    add("wide-bands", planted(300, 17), threshold=40, band_bits=32, band_count=2, auto_path=0)
    return c
