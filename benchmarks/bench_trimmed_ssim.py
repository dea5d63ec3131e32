#!/usr/bin/env python3
"""The SSIM re-check of trimmed pairs beside the only route to the same scores without it, in one process, the compared
calls alternating.  One JSON line per row, appended to --out as well (profiles/r18_trimmed_ssim.jsonl is the record).
Records only, no gate.

    python benchmarks/bench_trimmed_ssim.py --leg pairs    # (a) ke_ssim_pairs_boxed against ke_crop_pack + ke_ssim_pairs
    python benchmarks/bench_trimmed_ssim.py --leg crop     # (b) ke_crop_luma alone, beside ke_crop_pack on the same boxes

(a) Device-resident RGB pairs of 512 x 512 and of 4032 x 3024, image a as it lies against a box of image b: a letterbox (an
eighth of the rows off the top and the bottom, whole rows) and a frame (margins on all four sides, an odd first column).
The old route copies every b's box out with ke_crop_pack (3 B/px, into a buffer reserved beforehand) and scores the packed
crops with ke_ssim_pairs; the scores of the two routes are asserted bit-equal.  Both are timed on the host clock from one
synchronised state to the next, since ke_crop_pack lies outside the SSIM timer; ``ssim_timer_ms`` is KE_T_SSIM of the new
call (the crop is inside it).
(b) The same boxes, kernel time by HIP events (ke_last_kernel_ms kind 7 and kind 6): bytes read + bytes written over the time;
the streaming-read ceiling of profiles/r03_hbm_read.txt is 6.9 TB/s.

Each figure is the median of 5 timed calls after 2 untimed ones, with the lowest and the highest.  One GPU."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("pairs", "crop"), required=True)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604
SHAPES = ((512, 512, 256), (4032, 3024, 8))        # width, height, pairs
HBM_READ_TB_S = 6.9
T_TRIM_CROP, T_TRIM_LUMA, T_SSIM = 6, 7, 2


def boxes_of(w, h):
    return (("letterbox", (0, h // 8, w, h - h // 8)), ("frame", (w // 16 + 1, h // 8, w - w // 16 - 2, h - h // 8)))


def stats(ms):
    return {"median": float(np.median(ms)), "lowest": float(min(ms)), "highest": float(max(ms))}


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def corpus(ctx, w, h, n):
    """n synthetic RGB images back to back on the device: (pointer, bytes per image)."""
    img = w * h * 3
    px = ctx.malloc(n * img + 64)
    step = max(1, (64 << 20) // img)
    for first in range(0, n, step):
        ctx.synth_rgb(SEED, first, min(step, n - first), w, h, out=px + first * img)
    return px, img


def pairs_leg():
    ctx = _native.Context(0)
    for w, h, pairs in SHAPES:
        n = 2 * pairs
        px, img = corpus(ctx, w, h, n)
        packed = ctx.malloc(pairs * img + 64)                         # the old route's RGB crops of the b's
        ptrs = [px + i * img for i in range(n)]
        widths, heights = [w] * n, [h] * n
        pa, pb = list(range(0, n, 2)), list(range(1, n, 2))
        b_off = np.asarray([i * img for i in pb], np.uint64)
        for name, box in boxes_of(w, h):
            bw, bh = box[2] - box[0], box[3] - box[1]
            crop = (bw * bh * 3 + 15) & ~15
            out_off = np.arange(pairs, dtype=np.uint64) * np.uint64(crop)
            box_b = np.tile(np.asarray(box, np.int32), (pairs, 1))
            new_ms, old_ms, timer_ms = [], [], []
            for _ in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                ctx.crop_pack(px, b_off, [w] * pairs, [h] * pairs, 3, box_b, packed, out_off)
                old, old_status = ctx.ssim_pairs_on_device(ptrs[0::2] + [packed + int(o) for o in out_off], [w] * pairs + [bw] * pairs,
                                                           [h] * pairs + [bh] * pairs, 3, list(range(pairs)), list(range(pairs, 2 * pairs)))
                old_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                new, new_status = ctx.ssim_pairs_boxed_on_device(ptrs, widths, heights, 3, pa, pb, None, box_b)
                new_ms.append((time.perf_counter() - t0) * 1e3)
                timer_ms.append(ctx.last_kernel_ms(T_SSIM))
            assert not old_status.any() and not new_status.any()
            assert new.tolist() == old.tolist(), "the two routes disagree"
            o, m = stats(old_ms[args.warmup:]), stats(new_ms[args.warmup:])
            emit({"case": "pairs", "width": w, "height": h, "pairs": pairs, "box": name, "box_xyxy": list(box),
                  "crop_pack_then_ssim_pairs_ms": o, "ssim_pairs_boxed_ms": m, "ssim_timer_ms": stats(timer_ms[args.warmup:]),
                  "old_over_new": o["median"] / m["median"], "scores_bit_equal": True, "gpus": 1})
        ctx.free(packed)
        ctx.free(px)


def crop_leg():
    ctx = _native.Context(0)
    for w, h, n in SHAPES:
        px, img = corpus(ctx, w, h, n)
        dst = ctx.malloc(n * img + 64)
        src_off = np.arange(n, dtype=np.uint64) * np.uint64(img)
        for name, box in boxes_of(w, h):
            bw, bh = box[2] - box[0], box[3] - box[1]
            box_n = np.tile(np.asarray(box, np.int32), (n, 1))
            luma_off = np.arange(n, dtype=np.uint64) * np.uint64((bw * bh + 255) & ~255)
            pack_off = np.arange(n, dtype=np.uint64) * np.uint64((bw * bh * 3 + 255) & ~255)
            luma_ms, pack_ms = [], []
            for _ in range(args.warmup + args.reps):
                ctx.crop_luma(px, src_off, [w] * n, [h] * n, [3] * n, box_n, dst, luma_off)
                luma_ms.append(ctx.last_kernel_ms(T_TRIM_LUMA))
                ctx.crop_pack(px, src_off, [w] * n, [h] * n, 3, box_n, dst, pack_off)
                pack_ms.append(ctx.last_kernel_ms(T_TRIM_CROP))
            lm, pk = stats(luma_ms[args.warmup:]), stats(pack_ms[args.warmup:])
            moved, copied = n * bw * bh * 4, n * bw * bh * 6
            emit({"case": "crop_luma", "width": w, "height": h, "images": n, "channels": 3, "box": name, "box_xyxy": list(box),
                  "crop_luma_kernel_ms": lm, "bytes_in_plus_out": moved, "tb_per_s": moved / lm["median"] / 1e9,
                  "hbm_read_ceiling_tb_per_s": HBM_READ_TB_S, "share_of_ceiling": moved / lm["median"] / 1e9 / HBM_READ_TB_S,
                  "crop_pack_kernel_ms": pk, "crop_pack_bytes_in_plus_out": copied, "crop_pack_tb_per_s": copied / pk["median"] / 1e9,
                  "crop_pack_over_crop_luma": pk["median"] / lm["median"], "gpus": 1})
        ctx.free(dst)
        ctx.free(px)


{"pairs": pairs_leg, "crop": crop_leg}[args.leg]()
