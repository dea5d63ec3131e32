#!/usr/bin/env python3
"""Scan alone at several table sizes, back to back (HIP-event times of everything ke_hamming_scan launches, on
device-resident synthetic hash tables): where the per-tile rate of the large tables is lost at N = 100 000, and what the
bucket path costs beside the tile kernel.
    python benchmarks/scan_sizes.py [--mode auto|tiles|buckets] [--skew F ...] [--group G] [--parts P] [N ...]
--mode sets KE_SCAN_MODE before the context is made (the library reads it once per process).
--skew F: that fraction of the table is overwritten with identical hashes, in groups of G (--group, default 16) copies of one
hash each (identical images piling up in one bucket per band: F sets how many bucket pairs there are, G how long the
longest bucket is; F n (G - 1) / 2 of the pairs are edges).  Several values run one after the other at every N.
--parts P: time shard 0 of P only (one rank's share of a sharded scan).
tpairs_per_s / frac_of_fp4_peak are all-pairs EQUIVALENTS when the bucket path ran (path = 1): it visits far fewer pairs."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("auto", "tiles", "buckets"), default=None)
ap.add_argument("--skew", type=float, nargs="*", default=[0.0])
ap.add_argument("--group", type=int, default=16)
ap.add_argument("--parts", type=int, default=1)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("sizes", type=int, nargs="*")
args = ap.parse_args()
if args.mode:
    os.environ["KE_SCAN_MODE"] = args.mode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604
ctx = _native.Context(0)
sizes = args.sizes or [20_000, 50_000, 100_000, 200_000, 400_000, 1_000_000]
for n in sizes:
    for skew in args.skew:
        d = ctx.malloc(n * 8)
        ctx.synth_hashes(SEED, n, out=d)
        same = int(round(skew * n))
        h = np.empty(n, np.uint64)
        ctx.memcpy(h.ctypes.data, d, n * 8)
        if same:
            at = np.random.default_rng(SEED).choice(n, same, replace=False)
            h[at] = h[at[np.arange(same) // args.group * args.group]]
            ctx.memcpy(d, h.ctypes.data, n * 8)
        longest = max(int(np.unique((h >> np.uint64(16 * b)) & np.uint64(0xFFFF), return_counts=True)[1].max()) for b in range(4))
        ms, cap = [], None
        for _ in range(args.reps):
            edges, counters = ctx.hamming_scan(d, n, threshold=8, part_index=0, part_count=args.parts, capacity=cap)
            cap = max(1 << 16, 2 * n, len(edges))       # a skewed table's edges outgrow the default buffer: retry once, not every time
            ms.append(ctx.last_kernel_ms(1))
        ctx.free(d)
        med = float(np.median(ms[2:]))
        pairs = int(counters[0])
        print(json.dumps({"n": n, "mode": os.environ.get("KE_SCAN_MODE", "auto"), "path": ctx.last_scan_path(), "skew": skew, "group": args.group,
                          "parts": args.parts, "scan_ms_median": med, "scan_ms_min": float(min(ms)),
                          "scan_ms_max_after_warmup": float(max(ms[2:])), "edges": int(len(edges)),
                          "bucket_pairs": int(counters[3]), "longest_bucket": longest, "all_pairs_over_bucket_pairs": n * (n - 1) / 2 / max(1, int(counters[3])),
                          "tpairs_per_s": pairs / (med * 1e-3) / 1e12,
                          "frac_of_fp4_peak": pairs * 256 / (med * 1e-3) / 1e16}), flush=True)
