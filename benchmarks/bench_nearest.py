#!/usr/bin/env python3
"""The ranked search (ke_hamming_nearest) on device-resident tables of ke_synth_hashes: HIP-event time of its kernel
(ke_last_kernel_ms kind 9) and the wall time of the call, for n library hashes x m queries x k x max_distance.  Half of the
queries are library entries with 0..12 bits turned over, so that they have near neighbours; the other half are unrelated.
One JSON line per row, appended to --out as well (profiles/r20_nearest.jsonl is the record).

    python benchmarks/bench_nearest.py [--n N ...] [--m M ...] [--k K ...] [--max-distance D ...] [--check] [--out FILE]

Two yardsticks, both existing code run in this process:
  * ke_hamming_scan_cross through the all-pairs tile kernel (KE_SCAN_MODE=tiles, set here before the context is made: the
    library reads it once per process) on the table [library | queries] at threshold 8 -- the same n * m pairs on the matrix
    cores, answering a different question (an unordered edge set under a threshold and the band predicate);
  * NumPy on the host at n = 100 000, m = 64: what a caller has to do today for a ranked answer.
--check holds a 50-query sample of every row against the NumPy definition (xor, popcount, lexsort), so that a record cannot
come from a wrong kernel.  Each figure is the median of 5 timed calls after 2 untimed ones, with the lowest and the highest.
One GPU; nothing here runs on more than one."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[100_000, 1_000_000])
ap.add_argument("--m", type=int, nargs="*", default=[1, 64, 1_000, 10_000])
ap.add_argument("--k", type=int, nargs="*", default=[10, 1024])
ap.add_argument("--max-distance", type=int, nargs="*", default=[64, 12])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--check", action="store_true")
ap.add_argument("--no-yardsticks", action="store_true")
ap.add_argument("--tag", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
os.environ["KE_SCAN_MODE"] = "tiles"

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604


def stats(ms):
    return {"median": float(np.median(ms)), "lowest": float(min(ms)), "highest": float(max(ms))}


def emit(row):
    if args.tag:
        row["tag"] = args.tag
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def popcount64(x):
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def definition(hashes, queries, k, max_distance):
    """[(positions, distances)] per query: the entries within max_distance, the first k by (distance, position)"""
    out = []
    for q in queries:
        d = popcount64(hashes ^ q)
        pos = np.nonzero(d <= max_distance)[0]
        pos = pos[np.lexsort((pos, d[pos]))][:k]
        out.append((pos, d[pos]))
    return out


def make_queries(hashes, m):
    rng = np.random.default_rng([SEED, len(hashes), m])
    queries = rng.integers(0, 2**64, m, dtype=np.uint64)
    for at in range(0, m, 2):
        value = int(hashes[int(rng.integers(0, len(hashes)))])
        for b in rng.choice(64, int(rng.integers(0, 13)), replace=False):
            value ^= 1 << int(b)
        queries[at] = value
    return queries


ctx = _native.Context(0)
for n in args.n:
    hashes = ctx.synth_hashes(SEED, n)
    for m in args.m:
        queries = make_queries(hashes, m)
        table = ctx.malloc((n + m) * 8)                                  # [library | queries]: the cross scan's table, and ours
        ctx.memcpy(table, hashes, n * 8)
        ctx.memcpy(table + n * 8, queries, m * 8)
        tile_ms = None
        if not args.no_yardsticks:
            ms, cap = [], max(1 << 16, 2 * (n + m))
            for _ in range(args.warmup + args.reps):
                edges, counters = ctx.hamming_scan(table, n + m, threshold=8, capacity=cap, first_new=n, cross=True)
                cap = max(cap, len(edges))
                ms.append(ctx.last_kernel_ms(1))
            assert int(counters[0]) == n * m and ctx.last_scan_path() == 0
            tile_ms = stats(ms[args.warmup:])
            emit({"case": "tiles_cross", "n": n, "m": m, "threshold": 8, "edges": int(len(edges)), "scan_kernel_ms": tile_ms,
                  "pairs_per_s": n * m / (tile_ms["median"] * 1e-3), "gpus": 1})
            if n == 100_000 and m == 64:
                secs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    definition(hashes, queries, 10, 64)
                    secs.append(time.perf_counter() - t0)
                emit({"case": "numpy_host", "n": n, "m": m, "k": 10, "max_distance": 64, "ms": stats([s * 1e3 for s in secs]),
                      "pairs_per_s": n * m / float(np.median(secs))})
        for k in args.k:
            for max_distance in args.max_distance:
                kernel, call = [], []
                for _ in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    index, distance, count, within = ctx.hamming_nearest(table, table + n * 8, k=k, max_distance=max_distance, n=n, m=m)
                    call.append((time.perf_counter() - t0) * 1e3)
                    kernel.append(ctx.last_kernel_ms(9))
                checked = 0
                if args.check:
                    sample = np.unique(np.linspace(0, m - 1, min(m, 50)).astype(np.int64))
                    for q, (pos, d) in zip(sample, definition(hashes, queries[sample], k, max_distance)):
                        c = len(pos)
                        assert count[q] == c and np.array_equal(index[q, :c], pos) and np.array_equal(distance[q, :c], d), (n, m, k, max_distance, int(q))
                        assert (index[q, c:] == -1).all() and (distance[q, c:] == -1).all()
                        checked += 1
                row = {"case": "nearest", "n": n, "m": m, "k": k, "max_distance": max_distance, "nearest_kernel_ms": stats(kernel[args.warmup:]),
                       "nearest_call_ms": stats(call[args.warmup:]), "mean_count": float(count.mean()), "mean_within": float(within.mean()),
                       "checked_queries": checked, "gpus": 1}
                row["pairs_per_s"] = n * m / (row["nearest_kernel_ms"]["median"] * 1e-3)
                if tile_ms:
                    row["tiles_cross_kernel_ms"] = tile_ms["median"]
                    row["per_pair_vs_tiles"] = row["nearest_kernel_ms"]["median"] / tile_ms["median"]
                emit(row)
        ctx.free(table)
