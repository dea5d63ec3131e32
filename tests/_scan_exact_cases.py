"""What the exact scan (ke_hamming_scan_exact, ``exact=True``) is specified to return, in NumPy, and the tables its tests use --
shared by tests/test_scan_exact_cpu.py, tests/test_gpu_scan_exact.py and the GPU test's child process.

The definition: an edge is every pair (a < b) of the region with popcount(x_a ^ x_b) <= threshold, ids[a] != ids[b] and the
reference's fp64 size test ``smaller / larger >= ratio`` (skipped where a size is not positive); region 0 is all pairs,
1 is b >= first_new, 2 is a < first_new <= b; ``bands`` has bit min(k, 31) set for every band k < band_count in which the two
hashes agree and is 0 for a pair that shares none.  No band predicate decides anything."""
from __future__ import annotations

import numpy as np

from _scan_standin import OracleScanContext
from kobato_eyes_amd._native import EDGE_DTYPE

REGION_ALL, REGION_FROM, REGION_CROSS = 0, 1, 2
THRESHOLD = 8


def definition(hashes, *, ids=None, sizes=None, threshold=8, band_bits=16, band_count=4, size_ratio=0.0, region=REGION_ALL, first_new=0):
    """Sorted int64 rows (a, b, h, bands) of the exact edge set, by xor and np.bitwise_count over chunks of rows."""
    h = np.ascontiguousarray(hashes, dtype=np.uint64)
    n = len(h)
    first_new = int(first_new)
    assert region != REGION_ALL or first_new == 0
    rows = []
    for lo in range(0, n, 256):
        hi = min(lo + 256, n)
        d = np.bitwise_count(h[lo:hi, None] ^ h[None, :]).astype(np.int64)
        a, b = np.nonzero(d <= threshold)
        a = a + lo
        keep = a < b
        if ids is not None:
            keep &= np.asarray(ids)[a] != np.asarray(ids)[b]
        a, b = a[keep], b[keep]
        if sizes is not None and size_ratio and size_ratio > 0:
            sa, sb = np.asarray(sizes, np.int64)[a], np.asarray(sizes, np.int64)[b]
            small, large = np.minimum(sa, sb).astype(np.float64), np.maximum(sa, sb).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                ok = (sa <= 0) | (sb <= 0) | (small / large >= size_ratio)
            a, b = a[ok], b[ok]
        x = h[a] ^ h[b]
        mask = np.uint64((1 << band_bits) - 1) if band_bits < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
        bands = np.zeros(len(a), np.int64)
        for k in range(band_count):
            bands |= np.where((x >> np.uint64(k * band_bits)) & mask == 0, np.int64(1) << min(k, 31), 0)
        rows.append(np.stack([a, b, np.bitwise_count(x).astype(np.int64), bands], axis=1))
    out = np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)
    return in_region(sort_rows(out.reshape(-1, 4)), region, first_new)


def in_region(rows, region, first_new):
    """The rows of an all-pairs edge set that lie in a region: the three regions differ in nothing else."""
    if region == REGION_ALL:
        return rows
    keep = rows[:, 1] >= int(first_new)
    if region == REGION_CROSS:
        keep &= rows[:, 0] < int(first_new)
    return rows[keep]


def sort_rows(r):
    r = np.asarray(r, np.int64).reshape(-1, 4)
    return r[np.lexsort(r.T[::-1])]


def edge_rows(e):
    """EDGE_DTYPE records -> sorted int64 rows (a, b, h, bands)."""
    return sort_rows(np.stack([e["a"].astype(np.int64), e["b"].astype(np.int64), e["h"].astype(np.int64), e["bands"].astype(np.int64)], axis=1))


def region_pairs(n, region, first_new):
    """The region's pairs over all shards: what counters[0] must add up to."""
    f = int(first_new)
    if region == REGION_CROSS:
        return f * (n - f)
    return n * (n - 1) // 2 - f * (f - 1) // 2


def table(n, seed=0):
    """n hashes: the first third random bases, the rest copies of a base with 0..14 flipped bits (copy c of the run has
    c mod 15).  Every second copy has its first four flips in four different 16-bit bands, so from four flips on it shares no
    band with its base; the others flip where the generator says.  Also ids with repeats (every 7th entry carries its
    predecessor's) and sizes with zeros (every 5th) spread over a factor of four."""
    rng = np.random.default_rng(1000 + seed)
    n_base = max(1, n // 3) if n else 0
    h = np.zeros(n, np.uint64)
    h[:n_base] = rng.integers(0, 1 << 64, n_base, dtype=np.uint64)
    for c, i in enumerate(range(n_base, n)):
        flips = c % 15
        bits = rng.permutation(64)[:flips].tolist()
        if c % 2 and flips >= 4:
            bits[:4] = [16 * band + int(rng.integers(0, 16)) for band in range(4)]
            rest = [b for b in rng.permutation(64).tolist() if b not in bits[:4]]
            bits[4:] = rest[: flips - 4]
        word = int(h[c % n_base])
        for b in bits:
            word ^= 1 << b
        h[i] = np.uint64(word)
    order = rng.permutation(n)                     # copies do not sit in runs behind their bases
    h = h[order]
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    again = np.arange(7, n, 7)
    ids[again] = ids[again - 1]
    sizes = rng.integers(1000, 4000, n).astype(np.int64)
    sizes[::5] = 0
    return h, ids, sizes


def bandless_share(h, threshold=THRESHOLD):
    """(pairs within the threshold, those of them with a differing bit in every 16-bit band)."""
    rows = definition(h, threshold=threshold)
    return len(rows), int((rows[:, 3] == 0).sum())


class ExactScanContext(OracleScanContext):
    """The stand-in context of the view-scan tests with ``exact=True`` answered from the definition above; a banded call goes
    to the oracle as before.  ``exact_calls`` counts the exact ones."""

    def __init__(self):
        super().__init__()
        self.exact_calls = 0

    def hamming_scan(self, hashes, n, *, exact=False, **keywords):
        if not exact:
            return super().hamming_scan(hashes, n, **keywords)
        if keywords.get("bucket_pair_cap"):
            raise ValueError("exact=True takes no bucket_pair_cap: the cap is a property of buckets")
        self.exact_calls += 1
        first_new, cross = keywords.get("first_new"), keywords.get("cross", False)
        self.calls.append(dict(n=int(n), first_new=first_new, cross=cross, exact=True, hashes=np.array(hashes)))
        region = REGION_CROSS if cross else REGION_FROM if first_new else REGION_ALL
        rows = definition(hashes, ids=keywords.get("ids"), sizes=keywords.get("sizes"), threshold=keywords.get("threshold", 8),
                          band_bits=keywords.get("band_bits", 16), band_count=keywords.get("band_count", 4),
                          size_ratio=keywords.get("size_ratio", 0.0), region=region, first_new=int(first_new or 0))
        out = np.zeros(len(rows), EDGE_DTYPE)
        for k, name in enumerate(("a", "b", "h", "bands")):
            out[name] = rows[:, k]
        shared = int(sum(bin(int(b)).count("1") for b in rows[:, 3]))
        return out, np.array([region_pairs(int(n), region, int(first_new or 0)), shared, len(out), 0], np.uint64)


def pictures():
    """[(file name, PIL image)]: four smooth 96 x 96 pictures and edited copies of each -- brighter, a white patch, a black bar,
    shrunk to a third and back -- for the end-to-end test, which writes them as PNG and, the names say which, JPEG files."""
    from PIL import Image, ImageEnhance

    out = []
    yy, xx = np.mgrid[0:96, 0:96].astype(np.float64)
    for p in range(4):
        r = 127 + 120 * np.sin(xx / (9.0 + 4 * p) + p) * np.cos(yy / (13.0 + 3 * p))
        g = 127 + 120 * np.sin((xx + 2 * yy) / (17.0 + 5 * p))
        b = 127 + 120 * np.cos((xx * (p + 1) - yy) / 21.0)
        base = Image.fromarray(np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8), "RGB")
        patch = base.copy()
        patch.paste((255, 255, 255), (60, 10, 84, 30))
        bar = base.copy()
        bar.paste((0, 0, 0), (0, 84, 96, 96))
        out += [(f"p{p}_base.png", base), (f"p{p}_bright.png", ImageEnhance.Brightness(base).enhance(1.25)),
                (f"p{p}_patch.jpg", patch), (f"p{p}_bar.png", bar),
                (f"p{p}_third.jpg", base.resize((32, 32), Image.BILINEAR).resize((96, 96), Image.BILINEAR))]
    return out
