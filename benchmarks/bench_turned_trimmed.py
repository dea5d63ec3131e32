#!/usr/bin/env python3
"""The calls for copies that are both bordered and turned beside the only routes to the same information without them, in one
process, the compared calls alternating.  One JSON line per row, appended to --out as well (profiles/r19_turned_trimmed.jsonl is
the record).  Records only, no gate.

    python benchmarks/bench_turned_trimmed.py --leg hash [--images 100000]   # (a) ke_hash_images_turned_trimmed against ke_hash_images_turned + ke_hash_images_trimmed
    python benchmarks/bench_turned_trimmed.py --leg pairs                    # (b) ke_ssim_pairs_viewed against ke_crop_pack + ke_ssim_pairs_turned
    python benchmarks/bench_turned_trimmed.py --leg kernel                   # (c) ke_crop_turn_luma alone, beside ke_turn_luma and ke_crop_luma

(a) 512 x 512 RGB resident, the benchmark's synthetic corpus, with 0 %, 5 % and 100 % of the images letterboxed in place (the
first and last 64 rows black).  The two old calls, one after the other on the same batch, give the turned hashes, the boxes and the
trimmed pHash -- part of what the new call gives; the seven other hashes of the crop they do not give at all.  Host clock round
calls that end synchronised.
(b) Device-resident RGB pairs of 512 x 512 and of 4032 x 3024, image a as it lies against orientation k of a box of image b: a
letterbox (an eighth of the rows off the top and the bottom) and a frame (margins on all four sides, an odd first column), k = 1,
2, 4, 5 and a mix (1..7 in turn).  The old route copies every b's box out with ke_crop_pack (3 B/px, into a buffer reserved
beforehand) and scores a against the packed crop with ke_ssim_pairs_turned; the scores of the two routes are asserted bit-equal.
Host clock from one synchronised state to the next; ``ssim_timer_ms`` is KE_T_SSIM of the new call.
(c) The same boxes, kernel time by HIP events (ke_last_kernel_ms kind 8): bytes read + bytes written over the time, against the
6.9 TB/s streaming-read ceiling of profiles/r03_hbm_read.txt; beside it ke_turn_luma on unboxed images of the box's size (no
kind of its own: the host clock round the blocking call, as for ke_crop_turn_luma in that column) and, at k = 0, ke_crop_luma
(kind 7).

Each figure is the median of 5 timed calls after 2 untimed ones, with the lowest and the highest.  One GPU."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("hash", "pairs", "kernel"), required=True)
ap.add_argument("--images", type=int, default=None)
ap.add_argument("--tolerance", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604
SHAPES = ((512, 512, 256), (4032, 3024, 8))        # width, height, pairs
ORIENTATIONS = (("1", [1]), ("2", [2]), ("4", [4]), ("5", [5]), ("mix", [1, 2, 3, 4, 5, 6, 7]))
HBM_READ_TB_S = 6.9
BAR = 64
T_SSIM, T_TRIM_LUMA, T_VIEW_LUMA = 2, 7, 8


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
    step = max(1, (1 << 30) // img)
    for first in range(0, n, step):
        ctx.synth_rgb(SEED, first, min(step, n - first), w, h, out=px + first * img)
    return px, img


def hash_leg():
    ctx = _native.Context(0)
    n, w, h = args.images or 100_000, 512, 512
    px, img = corpus(ctx, w, h, n)
    offsets = np.arange(n, dtype=np.uint64) * np.uint64(img)
    widths, heights = np.full(n, w, np.int32), np.full(n, h, np.int32)
    a = lambda x: x.ctypes.data
    tn_old, st = np.zeros((n, 8), np.uint64), np.zeros(n, np.int32)
    ph_old, bx_old, has_old = np.zeros(n, np.uint64), np.zeros((n, 4), np.int32), np.zeros(n, np.uint8)
    tn, cut, bx, has = np.zeros((n, 8), np.uint64), np.zeros((n, 8), np.uint64), np.zeros((n, 4), np.int32), np.zeros(n, np.uint8)
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
        old_ms, new_ms, turned_ms, trimmed_ms = [], [], [], []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            ctx._check(ctx._lib.ke_hash_images_turned(ctx._h, px, a(offsets), a(widths), a(heights), 3, n, a(tn_old), a(st)), "ke_hash_images_turned")
            t1 = time.perf_counter()
            ctx._check(ctx._lib.ke_hash_images_trimmed(ctx._h, px, a(offsets), a(widths), a(heights), 3, n, args.tolerance, a(ph_old), a(bx_old),
                                                       a(has_old), a(st)), "ke_hash_images_trimmed")
            t2 = time.perf_counter()
            ctx._check(ctx._lib.ke_hash_images_turned_trimmed(ctx._h, px, a(offsets), a(widths), a(heights), 3, n, args.tolerance, a(tn), a(cut),
                                                              a(bx), a(has), a(st)), "ke_hash_images_turned_trimmed")
            t3 = time.perf_counter()
            turned_ms.append((t1 - t0) * 1e3)
            trimmed_ms.append((t2 - t1) * 1e3)
            old_ms.append((t2 - t0) * 1e3)
            new_ms.append((t3 - t2) * 1e3)
        assert not st.any()
        assert np.array_equal(tn, tn_old) and np.array_equal(bx, bx_old) and np.array_equal(has, has_old) and np.array_equal(cut[:, 0], ph_old)
        assert has[barred].all(), "a letterboxed image did not come back with its box"
        o, m = stats(old_ms[args.warmup:]), stats(new_ms[args.warmup:])
        emit({"case": "hash", "images": n, "width": w, "height": h, "share_letterboxed": share, "images_with_trimmed_hashes": int(has.sum()),
              "tolerance": args.tolerance, "hash_images_turned_ms": stats(turned_ms[args.warmup:]),
              "hash_images_trimmed_ms": stats(trimmed_ms[args.warmup:]), "turned_then_trimmed_ms": o, "hash_images_turned_trimmed_ms": m,
              "old_over_new": o["median"] / m["median"], "shared_outputs_equal": True, "gpus": 1})
    ctx.free(px)


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
            for label, ks in ORIENTATIONS:
                orient = [ks[i % len(ks)] for i in range(pairs)]
                new_ms, old_ms, timer_ms = [], [], []
                for _ in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    ctx.crop_pack(px, b_off, [w] * pairs, [h] * pairs, 3, box_b, packed, out_off)
                    old, old_status = ctx.ssim_pairs_turned_on_device(ptrs[0::2] + [packed + int(o) for o in out_off], [w] * pairs + [bw] * pairs,
                                                                      [h] * pairs + [bh] * pairs, 3, list(range(pairs)),
                                                                      list(range(pairs, 2 * pairs)), orient)
                    old_ms.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    new, new_status = ctx.ssim_pairs_viewed_on_device(ptrs, widths, heights, 3, pa, pb, None, box_b, orient)
                    new_ms.append((time.perf_counter() - t0) * 1e3)
                    timer_ms.append(ctx.last_kernel_ms(T_SSIM))
                assert not old_status.any() and not new_status.any()
                assert new.tolist() == old.tolist(), "the two routes disagree"
                o, m = stats(old_ms[args.warmup:]), stats(new_ms[args.warmup:])
                emit({"case": "pairs", "width": w, "height": h, "pairs": pairs, "box": name, "box_xyxy": list(box), "orientation": label,
                      "crop_pack_then_ssim_pairs_turned_ms": o, "ssim_pairs_viewed_ms": m, "ssim_timer_ms": stats(timer_ms[args.warmup:]),
                      "old_over_new": o["median"] / m["median"], "scores_bit_equal": True, "gpus": 1})
        ctx.free(packed)
        ctx.free(px)


def kernel_leg():
    ctx = _native.Context(0)
    for w, h, n in SHAPES:
        px, img = corpus(ctx, w, h, n)
        dst = ctx.malloc(n * img + 64)
        src_off = np.arange(n, dtype=np.uint64) * np.uint64(img)
        for name, box in boxes_of(w, h):
            bw, bh = box[2] - box[0], box[3] - box[1]
            box_n = np.tile(np.asarray(box, np.int32), (n, 1))
            luma_off = np.arange(n, dtype=np.uint64) * np.uint64((bw * bh + 255) & ~255)
            small_off = np.arange(n, dtype=np.uint64) * np.uint64(bw * bh * 3)          # unboxed images of the box's size, in the same bytes
            moved = n * bw * bh * 4
            for k in (0, 1, 2, 4, 5):
                view_ms, view_call_ms, turn_call_ms, crop_ms = [], [], [], []
                for _ in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    ctx.crop_turn_luma(px, src_off, [w] * n, [h] * n, [3] * n, box_n, [k] * n, dst, luma_off)
                    view_call_ms.append((time.perf_counter() - t0) * 1e3)
                    view_ms.append(ctx.last_kernel_ms(T_VIEW_LUMA))
                    t0 = time.perf_counter()
                    ctx.turn_luma(px, small_off, [bw] * n, [bh] * n, [3] * n, [k] * n, dst, luma_off)
                    turn_call_ms.append((time.perf_counter() - t0) * 1e3)
                    if k == 0:
                        ctx.crop_luma(px, src_off, [w] * n, [h] * n, [3] * n, box_n, dst, luma_off)
                        crop_ms.append(ctx.last_kernel_ms(T_TRIM_LUMA))
                vm = stats(view_ms[args.warmup:])
                emit({"case": "crop_turn_luma", "width": w, "height": h, "images": n, "channels": 3, "box": name, "box_xyxy": list(box),
                      "orientation": k, "crop_turn_luma_kernel_ms": vm, "bytes_in_plus_out": moved, "tb_per_s": moved / vm["median"] / 1e9,
                      "hbm_read_ceiling_tb_per_s": HBM_READ_TB_S, "share_of_ceiling": moved / vm["median"] / 1e9 / HBM_READ_TB_S,
                      "crop_turn_luma_call_ms": stats(view_call_ms[args.warmup:]),
                      "turn_luma_unboxed_same_size_call_ms": stats(turn_call_ms[args.warmup:]),
                      "crop_luma_kernel_ms": stats(crop_ms[args.warmup:]) if k == 0 else None, "gpus": 1})
        ctx.free(dst)
        ctx.free(px)


{"hash": hash_leg, "pairs": pairs_leg, "kernel": kernel_leg}[args.leg]()
