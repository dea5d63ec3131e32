"""ke_tiffc_decode throughput: decode + hash files/s at several batch sizes for 512 x 512 RGB TIFF files -- LZW and PackBits, each
with predictor none and 2, photograph-like and drawing-like content -- against two yardsticks taken in the same run: Pillow /
libtiff on the same files (one process, and through the batch hasher with KE_GPU_TIFF_COMPRESSED unset against set), and
ke_tiff_decode on the same pixels stored uncompressed (the ceiling).  One JSON line per measurement.

    python benchmarks/bench_tiffc.py [--sizes 4096,16384] [--repeats 5] [--distinct 32] [--seam-files 2048] [--only lzw]

The kernels' split (codes / copies / rows) comes from a kernel trace of one call: run this with --sizes 4096 --repeats 1
--seam-files 0 under the profiler.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [("lzw", "tiff_lzw", False), ("lzw_p2", "tiff_lzw", True), ("packbits", "packbits", False), ("packbits_p2", "packbits", True)]


def images(kind: str, distinct: int, side: int = 512) -> list:
    import _webp_cases as W

    rng = np.random.default_rng(5)
    out = []
    for _ in range(distinct):
        if kind == "drawing":
            out.append(W.content(rng, side, side, "drawing"))
        else:                                                    # smooth gradients with sensor-like noise
            out.append((W.content(rng, side, side, "smooth").astype(np.int16) + rng.integers(-5, 6, (side, side, 3))).clip(0, 255).astype(np.uint8))
    return out


def written(a: np.ndarray, compression, predictor: bool) -> bytes:
    b = io.BytesIO()
    how = {} if compression is None else {"compression": compression}
    if predictor:
        how["tiffinfo"] = {317: 2}
    Image.fromarray(a).save(b, "TIFF", **how)
    return b.getvalue()


def timed(fn, repeats: int):
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
    return wall


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--seam-files", type=int, default=2048)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import kobato_eyes_amd  # noqa: F401
    from kobato_eyes_amd import _native
    from kobato_eyes_amd import fastsig as K

    ctx = _native.get_context(0)
    sizes = [int(s) for s in args.sizes.split(",")]
    for kind in ("photo", "drawing"):
        pixels = images(kind, args.distinct)
        plain = [written(a, None, False) for a in pixels]
        for n in sizes:                                          # the ceiling: the same pixels, nothing to decode
            blobs = [plain[k % len(plain)] for k in range(n)]
            ctx.tiff_hash(blobs[:256])
            wall = timed(lambda: ctx.tiff_hash(blobs), args.repeats)
            print(json.dumps({"bench": "tiff_hash_uncompressed", "kind": kind, "files": n, "files_per_s_median": round(n / float(np.median(wall)), 1),
                              "files_per_s_lowest": round(n / max(wall), 1), "files_per_s_highest": round(n / min(wall), 1)}), flush=True)
        for name, compression, predictor in CONFIGS:
            if args.only and name != args.only:
                continue
            base = [written(a, compression, predictor) for a in pixels]
            t0 = time.perf_counter()
            for d in base:
                with Image.open(io.BytesIO(d)) as im:
                    im.load()
            pillow = len(base) / (time.perf_counter() - t0)
            print(json.dumps({"bench": "pillow_one_process", "kind": kind, "config": name, "files_per_s": round(pillow, 1),
                              "mean_file_bytes": int(np.mean([len(d) for d in base]))}), flush=True)
            for n in sizes:
                blobs = [base[k % len(base)] for k in range(n)]
                ctx.tiffc_hash(blobs[:256])                      # warm-up: buffers grown, code loaded
                wall, kernel = [], []
                for _ in range(args.repeats):
                    ctx.decode_kernel_ms = 0.0
                    t0 = time.perf_counter()
                    _, _, st = ctx.tiffc_hash(blobs)
                    wall.append(time.perf_counter() - t0)
                    kernel.append(ctx.decode_kernel_ms)
                    assert not np.asarray(st).any()
                print(json.dumps({"bench": "tiffc_hash", "kind": kind, "config": name, "files": n, "files_per_s_median": round(n / float(np.median(wall)), 1),
                                  "files_per_s_lowest": round(n / max(wall), 1), "files_per_s_highest": round(n / min(wall), 1),
                                  "decode_kernels_ms_median": round(float(np.median(kernel)), 2)}), flush=True)
            if args.seam_files <= 0:
                continue
            with tempfile.TemporaryDirectory() as tmp:           # the batch hasher over files on disk, the variable unset and set
                items = []
                for k in range(args.seam_files):
                    p = os.path.join(tmp, f"{k:05d}.tif")
                    with open(p, "wb") as f:
                        f.write(base[k % len(base)])
                    items.append((k, p))
                rows = {}
                for setting in ("0", "1", "0", "1"):             # each twice: the first pass also starts the decoder processes
                    os.environ["KE_GPU_TIFF_COMPRESSED"] = setting
                    t0 = time.perf_counter()
                    got = K.compute_signatures_mp(items)
                    took = time.perf_counter() - t0
                    assert len(got) == len(items) and rows.setdefault("rows", got) == got
                    rows.setdefault(setting, []).append(took)
                os.environ.pop("KE_GPU_TIFF_COMPRESSED", None)
                print(json.dumps({"bench": "batch_hasher_seam", "kind": kind, "config": name, "files": len(items),
                                  "files_per_s_variable_unset": round(len(items) / min(rows["0"]), 1),
                                  "files_per_s_variable_set": round(len(items) / min(rows["1"]), 1),
                                  "seconds_unset": [round(t, 3) for t in rows["0"]], "seconds_set": [round(t, 3) for t in rows["1"]]}), flush=True)


if __name__ == "__main__":
    main()
