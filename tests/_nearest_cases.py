"""The definition of ke_hamming_nearest in NumPy and the tables tests/test_gpu_nearest.py runs it on.

    S_q = { i : popcount(hashes[i] ^ queries[q]) <= max_distance, and not (ids and query_ids and ids[i] == query_ids[q]) }
    row q = the first min(k, |S_q|) of S_q by np.lexsort((position, distance))

``definition`` orders all rows at once with a stable argsort of the distances, entries outside S_q pushed past 64: a stable
sort by distance IS the order (distance, position); the first rows are held against np.lexsort itself on every call."""
from __future__ import annotations

import numpy as np

SEED = 20


def popcount64(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    x -= (x >> np.uint64(1)) & np.uint64(0x5555555555555555)
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.uint8)


def definition(hashes, queries, k: int, max_distance: int, ids=None, query_ids=None) -> tuple:
    """(index int64[m, k], distance int32[m, k], count int32[m], within int64[m], histogram uint32[m, 65])"""
    hashes, queries = np.asarray(hashes, np.uint64), np.asarray(queries, np.uint64)
    n, m = len(hashes), len(queries)
    index = np.full((m, k), -1, np.int64)
    distance = np.full((m, k), -1, np.int32)
    count = np.zeros(m, np.int32)
    within = np.zeros(m, np.int64)
    histogram = np.zeros((m, 65), np.uint32)
    both = ids is not None and query_ids is not None
    width = min(k, n)
    for lo in range(0, m, 8192):
        hi = min(m, lo + 8192)
        d = popcount64(hashes[None, :] ^ queries[lo:hi, None])
        keep = d <= max_distance
        if both:
            keep &= np.asarray(ids, np.int64)[None, :] != np.asarray(query_ids, np.int64)[lo:hi, None]
        pushed = np.where(keep, d, np.uint8(255))
        order = np.argsort(pushed, axis=1, kind="stable")[:, :width]
        within[lo:hi] = keep.sum(axis=1)
        count[lo:hi] = np.minimum(within[lo:hi], k)
        taken = np.arange(width)[None, :] < count[lo:hi, None]
        index[lo:hi, :width] = np.where(taken, order, -1)
        distance[lo:hi, :width] = np.where(taken, np.take_along_axis(d, order, axis=1).astype(np.int32), -1)
        rows = np.broadcast_to(np.arange(hi - lo)[:, None] * 65, d.shape)
        histogram[lo:hi] = np.bincount((rows + d)[keep], minlength=(hi - lo) * 65).reshape(hi - lo, 65)
        for q in range(lo, min(hi, lo + 3)):                                         # the words of the definition, row by row
            pos = np.nonzero(keep[q - lo])[0]
            pos = pos[np.lexsort((pos, d[q - lo][pos]))][:k]
            assert np.array_equal(index[q, :len(pos)], pos) and count[q] == len(pos)
    return index, distance, count, within, histogram


def flipped(rng, value: int, bits: int) -> int:
    """``value`` with ``bits`` distinct random bits turned over"""
    out = int(value)
    for b in rng.choice(64, bits, replace=False):
        out ^= 1 << int(b)
    return out


def random_table(n: int, m: int) -> tuple:
    """n random hashes, m random queries; min(n, 200) entries planted 0..12 bits from one of the queries"""
    rng = np.random.default_rng([SEED, n, m])
    hashes = rng.integers(0, 2**64, n, dtype=np.uint64)
    queries = rng.integers(0, 2**64, m, dtype=np.uint64)
    for at in rng.choice(n, min(n, 200), replace=False):
        hashes[at] = flipped(rng, queries[int(rng.integers(0, m))], int(rng.integers(0, 13)))
    return hashes, queries


def rotl(value: int, by: int) -> int:
    by %= 64
    return ((value << by) | (value >> (64 - by))) & (2**64 - 1) if by else value


def staircase(n: int, query: int) -> np.ndarray:
    """entry i differs from the query in exactly i mod 65 bits, the bit set rotated by i"""
    return np.array([query ^ rotl((1 << (i % 65)) - 1, i) for i in range(n)], np.uint64)


def at_distance(query: int, bits: int, salt: int) -> int:
    """a hash ``bits`` away from the query; different salts give different hashes where 0 < bits < 64"""
    return query ^ rotl((1 << bits) - 1, salt)
