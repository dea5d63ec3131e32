"""ke_tiffz_decode throughput: decode + hash files/s at several batch sizes for 512 x 512 RGB deflate TIFF files -- predictor none
and 2, photograph-like and drawing-like content, the files repeated from a few distinct ones -- against the yardsticks taken in
the same run on the same pixels: ke_tiffc_decode (LZW), ke_tiff_decode (uncompressed: the ceiling), ke_png_decode (the same
inflate at one lane per image instead of one per strip), Pillow / libtiff in one process, and the batch hasher over files on
disk with KE_GPU_TIFF_DEFLATE unset against set (after one pass each way that is not counted).  Median of --repeats with lowest
and highest everywhere but for Pillow in one process (one pass over the distinct files).  One JSON line per measurement.

    python benchmarks/bench_tiffz.py [--sizes 4096,16384] [--repeats 5] [--distinct 32] [--seam-files 2048] [--out FILE]

Not measured here: 65 536 files per call, files larger than 512 x 512, single-strip files.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tiffc import images, written  # noqa: E402

CONFIGS = [("deflate", "tiff_adobe_deflate", False), ("deflate_p2", "tiff_adobe_deflate", True)]


def png(a: np.ndarray) -> bytes:
    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG")
    return b.getvalue()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--seam-files", type=int, default=2048)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import kobato_eyes_amd  # noqa: F401
    from kobato_eyes_amd import _native
    from kobato_eyes_amd import fastsig as K

    ctx = _native.get_context(0)
    sizes = [int(s) for s in args.sizes.split(",")]
    sink = open(args.out, "a") if args.out else None

    def report(row: dict) -> None:
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def rate(bench: str, kind: str, config: str, hash_call, base: list) -> None:
        for n in sizes:
            blobs = [base[k % len(base)] for k in range(n)]
            hash_call(blobs[:256])                               # warm-up: buffers grown, code loaded
            wall, kernel = [], []
            for _ in range(args.repeats):
                ctx.decode_kernel_ms = 0.0
                t0 = time.perf_counter()
                _, _, st = hash_call(blobs)
                wall.append(time.perf_counter() - t0)
                kernel.append(ctx.decode_kernel_ms)
                assert not np.asarray(st).any()
            report({"bench": bench, "kind": kind, "config": config, "files": n, "repeats": args.repeats,
                    "files_per_s_median": round(n / float(np.median(wall)), 1), "files_per_s_lowest": round(n / max(wall), 1),
                    "files_per_s_highest": round(n / min(wall), 1), "decode_kernels_ms_median": round(float(np.median(kernel)), 2),
                    "mean_file_bytes": int(np.mean([len(d) for d in base]))})

    for kind in ("photo", "drawing"):
        pixels = images(kind, args.distinct)
        rate("tiff_hash_uncompressed", kind, "none", ctx.tiff_hash, [written(a, None, False) for a in pixels])
        rate("tiffc_hash", kind, "lzw_p2", ctx.tiffc_hash, [written(a, "tiff_lzw", True) for a in pixels])
        rate("png_hash", kind, "png", ctx.png_hash, [png(a) for a in pixels])
        for name, compression, predictor in CONFIGS:
            base = [written(a, compression, predictor) for a in pixels]
            t0 = time.perf_counter()
            for d in base:
                with Image.open(io.BytesIO(d)) as im:
                    im.load()
            report({"bench": "pillow_one_process", "kind": kind, "config": name, "files_per_s": round(len(base) / (time.perf_counter() - t0), 1),
                    "mean_file_bytes": int(np.mean([len(d) for d in base]))})
            rate("tiffz_hash", kind, name, ctx.tiffz_hash, base)
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
                # one pass each way that is not counted (it also starts the decoder processes), then --repeats each way, alternating
                for k, setting in enumerate(("0", "1") * (1 + args.repeats)):
                    os.environ["KE_GPU_TIFF_DEFLATE"] = setting
                    t0 = time.perf_counter()
                    got = K.compute_signatures_mp(items)
                    took = time.perf_counter() - t0
                    assert len(got) == len(items) and rows.setdefault("rows", got) == got
                    if k >= 2:
                        rows.setdefault(setting, []).append(took)
                os.environ.pop("KE_GPU_TIFF_DEFLATE", None)
                row = {"bench": "batch_hasher_seam", "kind": kind, "config": name, "files": len(items), "repeats": args.repeats}
                for setting, label in (("0", "unset"), ("1", "set")):
                    row.update({f"files_per_s_variable_{label}_median": round(len(items) / float(np.median(rows[setting])), 1),
                                f"files_per_s_variable_{label}_lowest": round(len(items) / max(rows[setting]), 1),
                                f"files_per_s_variable_{label}_highest": round(len(items) / min(rows[setting]), 1)})
                report(row)


if __name__ == "__main__":
    main()
