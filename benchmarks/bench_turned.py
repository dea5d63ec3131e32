#!/usr/bin/env python3
"""Turned pHashes and the cross scan beside the calls they stand next to, in the same process, alternating: HIP-event
times of everything each call launches (ke_last_kernel_ms) on device-resident inputs.  One JSON line per row, appended to
--out as well (profiles/r15_turned.jsonl is the record).  Records only, no gate.

    python benchmarks/bench_turned.py --leg hash [--images 100000]           # ke_hash_images_turned against ke_hash_uniform (pHash only), 512 x 512 RGB
    python benchmarks/bench_turned.py --leg scan --mode tiles|buckets|auto [--n N ...]
                                                                              # ke_hamming_scan_cross against ke_hamming_scan_from on [N | 7 N] at first_new = N
    python benchmarks/bench_turned.py --leg files --files DIR [--make 16384] # find_turned_duplicates on JPEG files of 512 x 512 (--make writes them first)

--mode sets KE_SCAN_MODE before the context is made (the library reads it once per process), so every mode is a process of
its own.  ke_hamming_scan_from on the same table and first_new is the only way to these edges without the cross scan; it also
visits the 24.5 N^2 pairs between two queries.  Each figure is the median of 5 timed calls after 2 untimed ones, with the
lowest and the highest.  One GPU; nothing here runs on more than one."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("hash", "scan", "files"), required=True)
ap.add_argument("--mode", choices=("auto", "tiles", "buckets"), default=None)
ap.add_argument("--images", type=int, default=100_000)
ap.add_argument("--n", type=int, nargs="*", default=[100_000, 1_000_000])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--files", default=None, help="a directory of image files")
ap.add_argument("--make", type=int, default=0, help="--leg files: first write this many 512 x 512 JPEG files (quality 90) into --files")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.mode:
    os.environ["KE_SCAN_MODE"] = args.mode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604


def stats(ms):
    return {"median": float(np.median(ms)), "lowest": float(min(ms)), "highest": float(max(ms))}


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def hash_leg():
    ctx = _native.Context(0)
    n, w, h = args.images, 512, 512
    img = w * h * 3
    px = ctx.malloc(n * img)
    step = 4096
    for first in range(0, n, step):                                   # the bench corpus, written in place
        ctx.synth_rgb(SEED, first, min(step, n - first), w, h, out=px + first * img)
    d_p, d_t = ctx.malloc(n * 8), ctx.malloc(n * 64)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(img)
    widths, heights = np.full(n, w, np.int32), np.full(n, h, np.int32)
    status = np.zeros(n, np.int32)
    ms_plain, ms_ragged, ms_turned = [], [], []
    for _ in range(args.warmup + args.reps):
        ctx._check(ctx._lib.ke_hash_uniform(ctx._h, px, n, w, h, 3, d_p, None), "ke_hash_uniform")
        ms_plain.append(ctx.last_kernel_ms(0))
        # the same images through the ragged entry the turned call shares its dispatch with
        ctx._check(ctx._lib.ke_hash_images(ctx._h, px, offsets.ctypes.data, widths.ctypes.data, heights.ctypes.data, 3, n, d_p, None,
                                           status.ctypes.data), "ke_hash_images")
        ms_ragged.append(ctx.last_kernel_ms(0))
        ctx._check(ctx._lib.ke_hash_images_turned(ctx._h, px, offsets.ctypes.data, widths.ctypes.data, heights.ctypes.data, 3, n, d_t,
                                                  status.ctypes.data), "ke_hash_images_turned")
        ms_turned.append(ctx.last_kernel_ms(0))
    plain, turned = np.zeros(n, np.uint64), np.zeros((n, 8), np.uint64)
    ctx.memcpy(plain, d_p, plain.nbytes)
    ctx.memcpy(turned, d_t, turned.nbytes)
    assert np.array_equal(turned[:, 0], plain), "column 0 is not the pHash"
    p, r, t = stats(ms_plain[args.warmup:]), stats(ms_ragged[args.warmup:]), stats(ms_turned[args.warmup:])
    emit({"case": "hash", "images": n, "width": w, "height": h, "bytes_per_image": img, "extra_bytes_per_image": 2048,
          "hash_uniform_phash_ms": p, "hash_images_phash_ms": r, "hash_images_turned_ms": t, "turned_over_plain": t["median"] / p["median"],
          "plain_tb_per_s": n * img / p["median"] / 1e9, "gpus": 1})
    for d in (px, d_p, d_t):
        ctx.free(d)


def scan_leg():
    ctx = _native.Context(0)
    for n_lib in args.n:
        n = 8 * n_lib
        d = ctx.malloc(n * 8)
        ctx.synth_hashes(SEED, n, out=d)
        cap = max(1 << 16, 2 * n)
        ms_cross, ms_from = [], []
        from_edges, from_path, from_error = None, None, None
        for _ in range(args.warmup + args.reps):                      # alternating, so that both see the same neighbours
            if from_error is None:
                try:
                    from_edges, _ = ctx.hamming_scan(d, n, threshold=8, capacity=cap, first_new=n_lib)
                    ms_from.append(ctx.last_kernel_ms(1))
                    from_path = ctx.last_scan_path()
                    cap = max(cap, len(from_edges))
                except RuntimeError as exc:                           # e.g. more tiles than one launch holds: recorded, not timed
                    from_error, from_edges = str(exc), None
            edges, counters = ctx.hamming_scan(d, n, threshold=8, capacity=cap, first_new=n_lib, cross=True)
            ms_cross.append(ctx.last_kernel_ms(1))
        if from_edges is not None:
            assert len(edges) == int((from_edges["a"] < n_lib).sum()), "the cross edges are not the scan from first_new's with a < first_new"
        assert int(counters[0]) == n_lib * (n - n_lib)
        c = stats(ms_cross[args.warmup:])
        f = stats(ms_from[args.warmup:]) if from_error is None else None
        emit({"case": "scan_cross", "library": n_lib, "queries": n - n_lib, "n": n, "first_new": n_lib,
              "mode": os.environ.get("KE_SCAN_MODE", "auto"), "path": ctx.last_scan_path(), "from_path": from_path,
              "cross_pairs": int(counters[0]), "from_pairs": n * (n - 1) // 2 - n_lib * (n_lib - 1) // 2, "bucket_pairs": int(counters[3]),
              "edges": int(len(edges)), "from_edges": None if from_edges is None else int(len(from_edges)), "cross_ms": c, "from_ms": f,
              "from_error": from_error, "from_over_cross": None if f is None else f["median"] / c["median"], "gpus": 1})
        ctx.free(d)


def files_leg():
    """find_turned_duplicates on files: wall clock around calls that end synchronised; the stored hashes are made beforehand."""
    from pathlib import Path

    from kobato_eyes_amd import api, fastsig
    from kobato_eyes_amd.scanner import DuplicateFile

    if args.make:
        from PIL import Image

        os.makedirs(args.files, exist_ok=True)
        ctx = _native.get_context(0)
        for first in range(0, args.make, 256):
            px = ctx.synth_rgb(SEED, first, min(256, args.make - first), 512, 512)
            for k, im in enumerate(px):
                Image.fromarray(im).save(os.path.join(args.files, f"f{first + k:06d}.jpg"), quality=90)
    paths = sorted(str(p) for p in Path(args.files).iterdir() if p.is_file())
    filled = fastsig.fast_fill_missing_signatures(":memory:", list(enumerate(paths)), apply_to_db=False)
    files = [DuplicateFile(fid, Path(paths[fid]), os.path.getsize(paths[fid]), 512, 512, int(ph) & ((1 << 64) - 1)) for fid, ph, _ in filled]
    turned_s, plain_s = [], []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        plain = api.find_duplicates(files)
        plain_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        clusters, matches = api.find_turned_duplicates(files)
        turned_s.append(time.perf_counter() - t0)
    emit({"case": "files", "files": len(files), "find_turned_duplicates_s": stats(turned_s[args.warmup:]),
          "find_duplicates_stored_hashes_s": stats(plain_s[args.warmup:]), "clusters": len(clusters), "plain_clusters": len(plain),
          "matches": len(matches), "gpus": 1})


{"hash": hash_leg, "scan": scan_leg, "files": files_leg}[args.leg]()
