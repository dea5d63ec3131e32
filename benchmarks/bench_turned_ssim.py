#!/usr/bin/env python3
"""The SSIM re-check of turned pairs beside the only route to the same scores without it, in one process, the compared
calls alternating.  One JSON line per row, appended to --out as well (profiles/r16_turned_ssim.jsonl is the record).
Records only, no gate.

    python benchmarks/bench_turned_ssim.py --leg pairs     # (a) ke_ssim_pairs_turned against ke_normalise_rgb + ke_ssim_pairs
    python benchmarks/bench_turned_ssim.py --leg turn      # (b) ke_turn_luma alone, bytes in + bytes out per second
    python benchmarks/bench_turned_ssim.py --leg fit       # what one fit launch costs at 4032 x 3024, by images and channels

(a) Device-resident RGB pairs of 512 x 512 and of 4032 x 3024, image a against orientation k of image b for k = 1, 2, 4, 5
and a mix of all eight.  The old route turns every b with ke_normalise_rgb under the EXIF orientation that is the same
permutation (a full RGB copy, into a buffer reserved beforehand) and scores the result with ke_ssim_pairs; the scores of the
two routes are asserted bit-equal.  Both are timed on the host clock from one synchronised state to the next, since
ke_normalise_rgb lies outside the SSIM timer; ``ssim_timer_ms`` is KE_T_SSIM of the new call (the turn is inside it).
(b) Orientation by orientation on the same images; the streaming-read ceiling of profiles/r03_hbm_read.txt is 6.9 TB/s.

The fit leg explains (a) at the large size: ke_fit_luma_uniform (one ke_launch_resize_group, BICUBIC, HIP-event time) for 8 and
16 images at one and three channels, to the three common sizes (a) meets, with the plan that ran.

Each figure is the median of 5 timed calls after 2 untimed ones, with the lowest and the highest.  One GPU."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("pairs", "turn", "fit"), required=True)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604
SHAPES = ((512, 512, 256), (4032, 3024, 8))        # width, height, pairs
# orientation k (turned.ORIENTATIONS) -> the EXIF orientation that is the same permutation (ke_normalise_rgb)
EXIF = (1, 2, 4, 3, 5, 6, 8, 7)
HBM_READ_TB_S = 6.9


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
        turned_rgb = ctx.malloc(pairs * img + 64)                     # the old route's RGB copies of the b's
        ptrs = [px + i * img for i in range(n)]
        widths, heights = [w] * n, [h] * n
        pa, pb = list(range(0, n, 2)), list(range(1, n, 2))
        b_off = np.asarray([i * img for i in pb], np.uint64)
        out_off = np.arange(pairs, dtype=np.uint64) * np.uint64(img)
        bw, bh, bc = np.full(pairs, w, np.int32), np.full(pairs, h, np.int32), np.full(pairs, 3, np.int32)
        for name, ks in (("1", [1]), ("2", [2]), ("4", [4]), ("5", [5]), ("mix", list(range(8)))):
            orient = [ks[j % len(ks)] for j in range(pairs)]
            exif = np.asarray([EXIF[k] for k in orient], np.int32)
            tw = [h if k & 4 else w for k in orient]
            th = [w if k & 4 else h for k in orient]
            new_ms, old_ms, timer_ms = [], [], []
            for _ in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                ctx._check(ctx._lib.ke_normalise_rgb(ctx._h, px, b_off.ctypes.data, bw.ctypes.data, bh.ctypes.data, bc.ctypes.data,
                                                     exif.ctypes.data, pairs, turned_rgb, out_off.ctypes.data), "ke_normalise_rgb")
                old, old_status = ctx.ssim_pairs_on_device(ptrs[0::2] + [turned_rgb + j * img for j in range(pairs)], [w] * pairs + tw,
                                                           [h] * pairs + th, 3, list(range(pairs)), list(range(pairs, 2 * pairs)))
                old_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                new, new_status = ctx.ssim_pairs_turned_on_device(ptrs, widths, heights, 3, pa, pb, orient)
                new_ms.append((time.perf_counter() - t0) * 1e3)
                timer_ms.append(ctx.last_kernel_ms(2))
            assert not old_status.any() and not new_status.any()
            assert new.tolist() == old.tolist(), "the two routes disagree"
            o, m = stats(old_ms[args.warmup:]), stats(new_ms[args.warmup:])
            emit({"case": "pairs", "width": w, "height": h, "pairs": pairs, "orientation": name, "normalise_then_ssim_pairs_ms": o,
                  "ssim_pairs_turned_ms": m, "ssim_timer_ms": stats(timer_ms[args.warmup:]), "old_over_new": o["median"] / m["median"],
                  "scores_bit_equal": True, "gpus": 1})
        ctx.free(turned_rgb)
        ctx.free(px)


def turn_leg():
    ctx = _native.Context(0)
    for w, h, n in SHAPES:
        px, img = corpus(ctx, w, h, n)
        plane = w * h
        dst = ctx.malloc(n * plane + 64)
        src_off = np.arange(n, dtype=np.uint64) * np.uint64(img)
        dst_off = np.arange(n, dtype=np.uint64) * np.uint64(plane)
        for k in range(8):
            ms = []
            for _ in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                ctx.turn_luma(px, src_off, [w] * n, [h] * n, [3] * n, [k] * n, dst, dst_off)
                ms.append((time.perf_counter() - t0) * 1e3)
            s = stats(ms[args.warmup:])
            moved = n * (img + plane)
            emit({"case": "turn_luma", "width": w, "height": h, "images": n, "channels": 3, "orientation": k, "ms": s, "bytes_in_plus_out": moved,
                  "tb_per_s": moved / s["median"] / 1e9, "hbm_read_ceiling_tb_per_s": HBM_READ_TB_S, "gpus": 1})
        ctx.free(dst)
        ctx.free(px)


def fit_leg():
    ctx = _native.Context(0)
    w, h = SHAPES[1][:2]
    for ch in (3, 1):
        for n in (8, 16):
            px, out = ctx.malloc(n * w * h * ch + 64), ctx.malloc(n * w * h + 64)
            for sw, sh, ow, oh in ((w, h, w, h), (h, w, h, h), (w, h, h, h)):
                ms = []
                for _ in range(args.warmup + args.reps):
                    ctx.fit_luma_uniform(px, n, sw, sh, ch, ow, oh, _native.FILTER_BICUBIC, out=out)
                    ms.append(ctx.last_kernel_ms(0))
                emit({"case": "fit_launch", "images": n, "channels": ch, "width": sw, "height": sh, "out_width": ow, "out_height": oh,
                      "kernel_ms": stats(ms[args.warmup:]), "resize_plan": list(ctx.last_resize_plan()), "gpus": 1})
            ctx.free(px)
            ctx.free(out)


{"pairs": pairs_leg, "turn": turn_leg, "fit": fit_leg}[args.leg]()
