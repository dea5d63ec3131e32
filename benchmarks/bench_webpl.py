"""ke_webpl_decode throughput: files/s at several batch sizes for 512 x 512 drawing-like and photograph-like lossless WebP files,
the decode kernels' time per compressed byte of the longest stream, and Pillow's rate on the same files (one process) for
comparison.  One JSON line per measurement.

    python benchmarks/bench_webpl.py [--sizes 4096,16384] [--repeats 5] [--distinct 64]
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def files(kind: str, distinct: int, side: int = 512) -> list:
    import _webp_cases as W

    rng = np.random.default_rng(5)
    out = []
    for _ in range(distinct):
        if kind == "drawing":
            a = W.content(rng, side, side, "drawing")
        else:                                                    # smooth gradients with sensor-like noise
            a = (W.content(rng, side, side, "smooth").astype(np.int16) + rng.integers(-5, 6, (side, side, 3))).clip(0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "WEBP", lossless=True, quality=75, method=4)
        out.append(buf.getvalue())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=64)
    args = ap.parse_args()
    import kobato_eyes_amd  # noqa: F401
    from kobato_eyes_amd import _native

    ctx = _native.get_context(0)
    for kind in ("drawing", "photo"):
        base = files(kind, args.distinct)
        t0 = time.perf_counter()
        for d in base:
            with Image.open(io.BytesIO(d)) as im:
                im.load()
        pillow = len(base) / (time.perf_counter() - t0)
        print(json.dumps({"bench": "pillow_one_process", "kind": kind, "files_per_s": round(pillow, 1),
                          "mean_file_bytes": int(np.mean([len(d) for d in base]))}), flush=True)
        for n in (int(s) for s in args.sizes.split(",")):
            blobs = [base[k % len(base)] for k in range(n)]
            ctx.webpl_hash(blobs[:256])                          # warm-up: buffers grown, code loaded
            wall, kernel = [], []
            for _ in range(args.repeats):
                ctx.decode_kernel_ms = 0.0
                t0 = time.perf_counter()
                _, _, st = ctx.webpl_hash(blobs)
                wall.append(time.perf_counter() - t0)
                kernel.append(ctx.decode_kernel_ms)
                assert not np.asarray(st).any()
            longest = max(len(d) for d in base)
            print(json.dumps({"bench": "webpl_hash", "kind": kind, "files": n, "files_per_s_median": round(n / float(np.median(wall)), 1),
                              "files_per_s_best": round(n / min(wall), 1), "decode_kernels_ms_median": round(float(np.median(kernel)), 2),
                              "longest_stream_bytes": longest,
                              "decode_kernels_us_per_byte_of_longest_stream": round(float(np.median(kernel)) * 1e3 / longest, 3)}), flush=True)


if __name__ == "__main__":
    main()
