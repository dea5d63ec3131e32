#!/usr/bin/env python3
"""JPEG files with restart intervals through ke_jpeg_decode + hash, with KE_JPEG_SPLIT_RESTARTS unset (one lane walks a file's
entropy-coded segment) and set (a lane per group of restart intervals), on the same files in the same process.  Quality 85,
4:2:0; median of ``--repeats`` calls with the lowest and highest; one JSON line per measurement.

    python benchmarks/bench_jpeg_restarts.py [--repeats 5] [--settings unset,set] [--rows 12mp_rows1,12mp_blocks4,12mp_no_dri,512_rows1]
                                             [--min-mcus 16,64,256] [--oversize jpeg|all]

rows: 4032x3024 with restart_marker_rows=1 at 128 and 1 024 files per call, the same pixels with restart_marker_blocks=4 and
without DRI at 128, 512x512 with restart_marker_rows=1 at 16 384.  ``--min-mcus``: the 128-file 12-megapixel rows with restarts
again, variable set, under each KE_JPEG_SPLIT_MIN_MCUS.  ``--oversize``: the file set of benchmarks/bench_oversize.py with its
JPEG files saved with restart_marker_rows=1 (``jpeg``: those files and the pairs among them alone) through refine_pairs with
KE_GPU_REFINE_OVERSIZE=1, under both settings; the answers must be equal.  A library without ke_jpeg_last_split (an older
build, for comparison: run this file from that tree with ``--settings unset``) reports no split counts."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SPLIT, MIN_MCUS = "KE_JPEG_SPLIT_RESTARTS", "KE_JPEG_SPLIT_MIN_MCUS"
ROWS = {      # name: (width, height, save options, files per call, distinct pictures)
    "12mp_rows1": (4032, 3024, {"restart_marker_rows": 1}, (128, 1024), 8),
    "12mp_blocks4": (4032, 3024, {"restart_marker_blocks": 4}, (128,), 8),
    "12mp_no_dri": (4032, 3024, {}, (128,), 8),
    "512_rows1": (512, 512, {"restart_marker_rows": 1}, (16384,), 256),
}


def picture(rng, w: int, h: int) -> Image.Image:
    """A small random image enlarged, with grain: photograph-like, cheap to make."""
    base = Image.fromarray(rng.integers(0, 256, (max(2, h // 64), max(2, w // 64), 3), dtype=np.uint8))
    big = np.asarray(base.resize((w, h), Image.Resampling.BICUBIC))
    return Image.fromarray(np.minimum(big, 247) + rng.integers(0, 9, (h, w, 1), dtype=np.uint8))


def set_env(split: bool, min_mcus=None) -> None:
    for name, value in ((SPLIT, "1" if split else None), (MIN_MCUS, None if min_mcus is None else str(min_mcus))):
        os.environ.pop(name, None)
        if value is not None:
            os.environ[name] = value


def measure(ctx, blobs, repeats: int):
    ph, _, st = ctx.jpeg_hash(blobs, want_dhash=False)                     # warm-up: buffers grown
    assert (st == 0).all()
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ph2, _, st = ctx.jpeg_hash(blobs, want_dhash=False)
        wall.append(time.perf_counter() - t0)
        assert (st == 0).all() and np.array_equal(ph, ph2)
    split = ctx.jpeg_last_split() if hasattr(ctx, "jpeg_last_split") else None
    return wall, split, ph


def report(out, **row) -> None:
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timing(wall, n=None) -> dict:
    med = float(np.median(wall))
    d = {"seconds_median": round(med, 4), "seconds_min": round(min(wall), 4), "seconds_max": round(max(wall), 4), "repeats": len(wall)}
    if n:
        d.update(images_per_s_median=round(n / med, 1), images_per_s_lowest=round(n / max(wall), 1), images_per_s_highest=round(n / min(wall), 1))
    return d


def oversize(K, args) -> None:
    import bench_oversize as B

    Image.MAX_IMAGE_PIXELS = None
    rng = np.random.default_rng(9)
    keep = [k for k, f in enumerate(B.FILES) if args.oversize == "all" or f[3] == "JPEG"]
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for k in keep:
            name, w, h, fmt, options = B.FILES[k]
            options = dict(options, restart_marker_rows=1) if fmt == "JPEG" else options
            paths[k] = os.path.join(tmp, name + (".jpg" if fmt == "JPEG" else ".png"))
            B.picture(rng, w, h, flat=fmt == "PNG").save(paths[k], fmt, **options)
        pairs = [(a, b, paths[a], paths[b]) for a, b in B.PAIRS if a in paths and b in paths]
        os.environ["KE_GPU_REFINE_OVERSIZE"] = "1"
        answers = {}
        for setting in args.settings:
            set_env(setting == "set")
            stats: dict = {}
            answers[setting] = K.refine_pairs(pairs, io_workers=args.io_workers, stats=stats)      # warm-up
            wall = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                K.refine_pairs(pairs, io_workers=args.io_workers)
                wall.append(time.perf_counter() - t0)
            report(args.out, bench="refine_pairs_oversize_restart_rows1", files=[B.FILES[k][0] for k in keep], pairs=len(pairs), KE_GPU_REFINE_OVERSIZE="1",
                   KE_JPEG_SPLIT_RESTARTS=setting, io_workers=args.io_workers, gpu_oversize=stats.get("gpu_oversize", 0), **timing(wall))
        if len(answers) == 2:
            assert answers["unset"] == answers["set"], "the two settings disagree"
        del os.environ["KE_GPU_REFINE_OVERSIZE"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--settings", default="unset,set")
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--min-mcus", default="", help="e.g. 16,64,256: the 128-file 12-megapixel rows with restarts under each minimum")
    ap.add_argument("--oversize", choices=["", "jpeg", "all"], default="")
    ap.add_argument("--io-workers", type=int, default=8)
    ap.add_argument("--out", default="", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    args.settings = [s for s in args.settings.split(",") if s]
    assert set(args.settings) <= {"unset", "set"}
    import kobato_eyes_amd as K
    from kobato_eyes_amd import _native

    ctx = _native.get_context(0)
    for name in [r for r in args.rows.split(",") if r]:
        w, h, options, per_call, distinct = ROWS[name]
        rng = np.random.default_rng([12, w, h])
        pictures = [picture(rng, w, h) for _ in range(distinct)]

        def encode(im):
            b = io.BytesIO()
            im.save(b, "JPEG", quality=85, subsampling=2, **options)
            return b.getvalue()

        with ThreadPoolExecutor(16) as ex:
            files = list(ex.map(encode, pictures))
        del pictures
        for n in per_call:
            blobs = [files[k % distinct] for k in range(n)]
            hashes = {}
            for setting in args.settings:
                set_env(setting == "set")
                wall, split, hashes[setting] = measure(ctx, blobs, args.repeats)
                report(args.out, bench="jpeg_decode_hash_restarts", row=name, width=w, height=h, files_per_call=n, compressed_mb=round(sum(map(len, blobs)) / 1e6, 1),
                       KE_JPEG_SPLIT_RESTARTS=setting, files_split_lanes=split, **timing(wall, n))
            assert all(np.array_equal(v, hashes[args.settings[0]]) for v in hashes.values()), "the settings disagree"
            if args.min_mcus and n == 128 and options:
                for m in [int(v) for v in args.min_mcus.split(",")]:
                    set_env(True, m)
                    wall, split, ph = measure(ctx, blobs, args.repeats)
                    assert np.array_equal(ph, hashes[args.settings[0]])
                    report(args.out, bench="jpeg_decode_hash_restarts_min_mcus", row=name, files_per_call=n, KE_JPEG_SPLIT_MIN_MCUS=m, files_split_lanes=split,
                           **timing(wall, n))
        set_env(False)
    if args.oversize:
        oversize(K, args)
    set_env(False)


if __name__ == "__main__":
    main()
