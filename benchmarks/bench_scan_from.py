#!/usr/bin/env python3
"""The scan from first_new (ke_hamming_scan_from) beside the full scan (ke_hamming_scan) and the cross scan
(ke_hamming_scan_cross, same first_new) of the same table, in the same
process, alternating: HIP-event times of everything each call launches (ke_last_kernel_ms), on device-resident tables of
ke_synth_hashes.  One JSON line per row, appended to --out as well (profiles/r13_scan_from.jsonl is the record).

    python benchmarks/bench_scan_from.py [--mode tiles|auto|buckets] [--n N ...] [--m M ...] [--out FILE]
    python benchmarks/bench_scan_from.py --full-only [--root TREE] [--tag NAME]      # ke_hamming_scan alone, e.g. of another build
    python benchmarks/bench_scan_from.py --files DIR [--added K]                     # find_new_duplicates with ssim_threshold

--mode sets KE_SCAN_MODE before the context is made (the library reads it once per process), so every mode is a process
of its own.  m = n - first_new; the default rows are n = 100 000 and 1 000 000 with m in {1 000, 10 000, n / 10, n / 2}.
Each figure is the median of 5 timed calls after 2 untimed ones, with the lowest and the highest.  One GPU; nothing here
runs on more than one.  The --files leg has not been run yet."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("auto", "tiles", "buckets"), default=None)
ap.add_argument("--n", type=int, nargs="*", default=[100_000, 1_000_000])
ap.add_argument("--m", type=int, nargs="*", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--full-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package is timed")
ap.add_argument("--tag", default="")
ap.add_argument("--out", default=None)
ap.add_argument("--files", default=None, help="a directory of image files: time find_new_duplicates with ssim_threshold on them")
ap.add_argument("--added", type=int, default=100, help="--files: how many of the files (the last ones by name) are the added set")
args = ap.parse_args()
if args.mode:
    os.environ["KE_SCAN_MODE"] = args.mode

sys.path.insert(0, args.root)
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604
TILE = 1024


def region_tiles(n: int, f: int) -> int:
    """csrc/ke_scan_region.h: the first `rect` row blocks own ncc - cc0 chunks each, the ones below their triangle rows."""
    if f >= n:
        return 0
    nb = (n + TILE - 1) // TILE
    tri = lambda rb: rb * nb - rb * (rb - 1) // 2
    rect = min(nb, f // TILE + 1)
    return rect * (nb - f // TILE) + tri(nb) - tri(rect)


def stats(ms):
    return {"median": float(np.median(ms)), "lowest": float(min(ms)), "highest": float(max(ms))}


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def files_leg():
    """find_new_duplicates against find_duplicates with ssim_threshold on real files: wall clock around calls that end
    synchronised, hashes computed once beforehand."""
    from kobato_eyes_amd import api, fastsig
    from kobato_eyes_amd.scanner import DuplicateFile
    from pathlib import Path
    from PIL import Image

    paths = sorted(str(p) for p in Path(args.files).iterdir() if p.is_file())
    filled = fastsig.fast_fill_missing_signatures(":memory:", list(enumerate(paths)), apply_to_db=False)
    files = []
    for fid, ph, _ in filled:
        with Image.open(paths[fid]) as im:
            w, h = im.size
        files.append(DuplicateFile(fid, Path(paths[fid]), os.path.getsize(paths[fid]), w, h, int(ph) & ((1 << 64) - 1)))
    library, added = files[:-args.added], files[-args.added:]
    for name, call in (("find_duplicates", lambda: api.find_duplicates(files, ssim_threshold=0.9)),
                       ("find_new_duplicates", lambda: api.find_new_duplicates(library, added, ssim_threshold=0.9))):
        t0 = time.perf_counter()
        clusters = call()
        emit({"case": "files", "call": name, "files": len(files), "added": len(added), "seconds": time.perf_counter() - t0,
              "clusters": len(clusters), "gpus": 1})


if args.files:
    files_leg()
    sys.exit(0)

ctx = _native.Context(0)
for n in args.n:
    d = ctx.malloc(n * 8)
    ctx.synth_hashes(SEED, n, out=d)
    cap = max(1 << 16, 2 * n)
    if args.full_only:
        ms = []
        for k in range(args.warmup + args.reps):
            edges, counters = ctx.hamming_scan(d, n, threshold=8, capacity=cap)
            cap = max(cap, len(edges))
            ms.append(ctx.last_kernel_ms(1))
        emit({"case": "full_only", "tag": args.tag, "n": n, "mode": os.environ.get("KE_SCAN_MODE", "auto"), "path": ctx.last_scan_path(),
              "edges": int(len(edges)), "full_ms": stats(ms[args.warmup:]), "gpus": 1})
        ctx.free(d)
        continue
    for m in sorted(set(args.m or [1_000, 10_000, n // 10, n // 2])):
        f = n - m
        ms_from, ms_full, ms_cross = [], [], []
        for k in range(args.warmup + args.reps):                      # alternating, so that all see the same neighbours
            full_edges, full_counters = ctx.hamming_scan(d, n, threshold=8, capacity=cap)
            ms_full.append(ctx.last_kernel_ms(1))
            full_path = ctx.last_scan_path()
            cross_edges, _ = ctx.hamming_scan(d, n, threshold=8, capacity=cap, first_new=f, cross=True)
            ms_cross.append(ctx.last_kernel_ms(1))
            cross_path = ctx.last_scan_path()
            edges, counters = ctx.hamming_scan(d, n, threshold=8, capacity=cap, first_new=f)
            ms_from.append(ctx.last_kernel_ms(1))
            cap = max(cap, len(full_edges))
        assert len(edges) == int((full_edges["b"] >= f).sum()), "the region's edges are not the full scan's with b >= first_new"
        assert len(cross_edges) == int(((full_edges["a"] < f) & (full_edges["b"] >= f)).sum()), "the cross edges are not the full scan's with a < first_new <= b"
        fr, fu = stats(ms_from[args.warmup:]), stats(ms_full[args.warmup:])
        emit({"case": "scan_from", "tag": args.tag, "n": n, "m": m, "first_new": f, "mode": os.environ.get("KE_SCAN_MODE", "auto"),
              "path": ctx.last_scan_path(), "full_path": full_path, "cross_path": cross_path, "cross_edges": int(len(cross_edges)),
              "cross_ms": stats(ms_cross[args.warmup:]), "region_pairs": int(counters[0]),
              "tiles": region_tiles(n, f), "full_tiles": region_tiles(n, 0), "edges": int(len(edges)), "full_edges": int(len(full_edges)),
              "bucket_pairs": int(counters[3]), "from_ms": fr, "full_ms": fu, "full_over_from": fu["median"] / fr["median"], "gpus": 1})
    ctx.free(d)
