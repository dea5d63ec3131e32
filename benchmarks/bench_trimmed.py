#!/usr/bin/env python3
"""The content-box kernel and the trimmed hash call beside the pHash pass of the same batch, in the same process,
alternating: HIP-event times of what each call launches (ke_last_kernel_ms; kind 5 = the box kernel, 6 = the crop kernel of
the last chunk, 0 = the hash kernels) on device-resident inputs, and host clocks round calls that end synchronised.  One
JSON line per row, appended to --out as well (profiles/r17_trimmed.jsonl is the record).  Records only, no gate.

    python benchmarks/bench_trimmed.py --leg boxes [--images 100000]          # ke_content_boxes against ke_hash_uniform (pHash only), 512 x 512 RGB
    python benchmarks/bench_trimmed.py --leg trimmed [--images 100000]        # ke_hash_images_trimmed with 0 %, 5 % and 100 % of the images letterboxed
    python benchmarks/bench_trimmed.py --leg large [--images 125]             # both kernels on 4032 x 3024 RGB
    python benchmarks/bench_trimmed.py --leg files --files DIR [--make 4096]  # find_trimmed_duplicates on JPEG files of 512 x 512 (--make writes them first)

The corpus is the benchmark's synthetic one, which has no borders: the box kernel reads every pixel whatever it finds.  A
letterboxed image has its first and last 64 rows set to black in place.  Bytes over time is the image bytes read once over
the box kernel's time, against the 6.9 TB/s streaming-read ceiling the README quotes.  Each figure is the median of 5 timed
calls after 2 untimed ones, with the lowest and the highest.  One GPU; nothing here runs on more than one."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("boxes", "trimmed", "large", "files"), required=True)
ap.add_argument("--images", type=int, default=None)
ap.add_argument("--tolerance", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--files", default=None, help="a directory of image files")
ap.add_argument("--make", type=int, default=0, help="--leg files: first write this many 512 x 512 JPEG files (quality 90) into --files, every fourth a letterboxed copy of the one before")
ap.add_argument("--out", default=None)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604
READ_CEILING_TB_S = 6.9
BAR = 64                     # rows of a letterbox bar


def stats(ms):
    return {"median": float(np.median(ms)), "lowest": float(min(ms)), "highest": float(max(ms))}


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def corpus(ctx, n, w, h):
    img = w * h * 3
    px = ctx.malloc(n * img)
    step = max(1, (1 << 30) // img)
    for first in range(0, n, step):                                   # the bench corpus, written in place
        ctx.synth_rgb(SEED, first, min(step, n - first), w, h, out=px + first * img)
    return px, img


def box_and_hash(ctx, px, n, w, h, img, case):
    """ke_content_boxes next to the pHash pass of the same batch."""
    d_p = ctx.malloc(n * 8)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(img)
    widths, heights = np.full(n, w, np.int32), np.full(n, h, np.int32)
    boxes, status = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    ms_hash, ms_box, s_box = [], [], []
    for _ in range(args.warmup + args.reps):
        ctx._check(ctx._lib.ke_hash_uniform(ctx._h, px, n, w, h, 3, d_p, None), "ke_hash_uniform")
        ms_hash.append(ctx.last_kernel_ms(0))
        t0 = time.perf_counter()
        ctx._check(ctx._lib.ke_content_boxes(ctx._h, px, offsets.ctypes.data, widths.ctypes.data, heights.ctypes.data, 3, n, args.tolerance,
                                             boxes.ctypes.data, status.ctypes.data), "ke_content_boxes")
        s_box.append((time.perf_counter() - t0) * 1e3)
        ms_box.append(ctx.last_kernel_ms(5))
    assert not status.any()
    p, b, c = stats(ms_hash[args.warmup:]), stats(ms_box[args.warmup:]), stats(s_box[args.warmup:])
    tb_s = n * img / b["median"] / 1e9
    emit({"case": case, "images": n, "width": w, "height": h, "bytes_per_image": img, "tolerance": args.tolerance,
          "hash_uniform_phash_ms": p, "content_boxes_kernel_ms": b, "content_boxes_call_ms": c, "box_over_phash": b["median"] / p["median"],
          "box_tb_per_s": tb_s, "box_share_of_read_ceiling": tb_s / READ_CEILING_TB_S, "phash_tb_per_s": n * img / p["median"] / 1e9,
          "images_with_a_box": int((boxes[:, 2] > 0).sum()), "gpus": 1})
    ctx.free(d_p)


def boxes_leg():
    ctx = _native.Context(0)
    n, w, h = args.images or 100_000, 512, 512
    px, img = corpus(ctx, n, w, h)
    box_and_hash(ctx, px, n, w, h, img, "boxes")
    ctx.free(px)


def large_leg():
    ctx = _native.Context(0)
    n, w, h = args.images or 125, 4032, 3024
    px, img = corpus(ctx, n, w, h)
    box_and_hash(ctx, px, n, w, h, img, "boxes_large")
    ctx.free(px)


def trimmed_leg():
    ctx = _native.Context(0)
    n, w, h = args.images or 100_000, 512, 512
    px, img = corpus(ctx, n, w, h)
    d_p = ctx.malloc(n * 8)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(img)
    widths, heights = np.full(n, w, np.int32), np.full(n, h, np.int32)
    ph, boxes = np.zeros(n, np.uint64), np.zeros((n, 4), np.int32)
    has, status = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    bar = np.zeros(BAR * w * 3, np.uint8)
    barred = np.zeros(n, bool)
    for share in (0.0, 0.05, 1.0):
        want = np.zeros(n, bool)
        if share > 0:
            want[np.arange(0, n, round(1 / share))] = True
        for i in np.nonzero(want & ~barred)[0]:                           # letterbox in place: the first and last BAR rows black
            ctx.memcpy(px + int(i) * img, bar, bar.nbytes)
            ctx.memcpy(px + int(i) * img + (h - BAR) * w * 3, bar, bar.nbytes)
        barred |= want
        ms_hash, s_call, ms_box, ms_crop, ms_crop_hash = [], [], [], [], []
        for _ in range(args.warmup + args.reps):
            ctx._check(ctx._lib.ke_hash_uniform(ctx._h, px, n, w, h, 3, d_p, None), "ke_hash_uniform")
            ms_hash.append(ctx.last_kernel_ms(0))
            t0 = time.perf_counter()
            ctx._check(ctx._lib.ke_hash_images_trimmed(ctx._h, px, offsets.ctypes.data, widths.ctypes.data, heights.ctypes.data, 3, n,
                                                       args.tolerance, ph.ctypes.data, boxes.ctypes.data, has.ctypes.data, status.ctypes.data),
                       "ke_hash_images_trimmed")
            s_call.append((time.perf_counter() - t0) * 1e3)
            ms_box.append(ctx.last_kernel_ms(5))
            ms_crop.append(ctx.last_kernel_ms(6))
            ms_crop_hash.append(ctx.last_kernel_ms(0))
        assert not status.any()
        assert has[barred].all() and (boxes[barred][:, [1, 3]] == [BAR, h - BAR]).all(), "a letterboxed image did not come back with its box"
        emit({"case": "trimmed", "images": n, "width": w, "height": h, "share_letterboxed": share, "images_with_a_trimmed_hash": int(has.sum()),
              "tolerance": args.tolerance, "hash_uniform_phash_ms": stats(ms_hash[args.warmup:]), "hash_images_trimmed_call_ms": stats(s_call[args.warmup:]),
              "content_boxes_kernel_ms": stats(ms_box[args.warmup:]),
              "last_chunk_crop_kernel_ms": stats(ms_crop[args.warmup:]) if has.any() else None,
              "last_chunk_hash_kernels_ms": stats(ms_crop_hash[args.warmup:]) if has.any() else None,
              "call_over_phash": float(np.median(s_call[args.warmup:]) / np.median(ms_hash[args.warmup:])), "gpus": 1})
    for d in (px, d_p):
        ctx.free(d)


def files_leg():
    """find_trimmed_duplicates on files: wall clock around calls that end synchronised; the stored hashes are made beforehand."""
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
                if (first + k) % 4 == 3:                                  # the picture before, letterboxed on a taller canvas
                    canvas = np.zeros((512 + 2 * BAR, 512, 3), np.uint8)
                    canvas[BAR:BAR + 512] = px[k - 1]
                    im = canvas
                Image.fromarray(im).save(os.path.join(args.files, f"f{first + k:06d}.jpg"), quality=90)
    paths = sorted(str(p) for p in Path(args.files).iterdir() if p.is_file())
    filled = fastsig.fast_fill_missing_signatures(":memory:", list(enumerate(paths)), apply_to_db=False)
    files = [DuplicateFile(fid, Path(paths[fid]), os.path.getsize(paths[fid]), 512, 512, int(ph) & ((1 << 64) - 1)) for fid, ph, _ in filled]
    trimmed_s, plain_s = [], []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        plain = api.find_duplicates(files)
        plain_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        clusters, matches = api.find_trimmed_duplicates(files, tolerance=args.tolerance)
        trimmed_s.append(time.perf_counter() - t0)
    emit({"case": "files", "files": len(files), "tolerance": args.tolerance, "find_trimmed_duplicates_s": stats(trimmed_s[args.warmup:]),
          "find_duplicates_stored_hashes_s": stats(plain_s[args.warmup:]), "clusters": len(clusters), "plain_clusters": len(plain),
          "matches": len(matches), "gpus": 1})


{"boxes": boxes_leg, "trimmed": trimmed_leg, "large": large_leg, "files": files_leg}[args.leg]()
