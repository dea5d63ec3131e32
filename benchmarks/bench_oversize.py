"""refine_pairs over files of 8 192 px and more, with KE_GPU_REFINE_OVERSIZE unset (the loader decodes and shrinks them on host
threads: the yardstick) and set (decoded at the draft scale, reduced and resampled on the device), in the same run on the same
files and pairs.  The answers of the two routes must be equal.  Medians of ``--repeats`` runs with the lowest and highest; one
JSON line per measurement.

    python benchmarks/bench_oversize.py [--repeats 5] [--io-workers 8]

``--trace`` instead says where such a call's time goes, on the first three files (two pairs) alone: under either setting, twice,
the whole call next to what ``KE_TRACE=1`` reports the JPEG decode call waiting for its kernels, and the loader by itself on one
thread over the same files.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import re
import sys
import tempfile
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, width, height, format, save options): an A3 scan at 600 dpi, two camera files, a panorama, a strip page
FILES = (
    ("camera_50mp", 8192, 6144, "JPEG", {"quality": 90, "subsampling": 2}),
    ("camera_50mp_b", 8192, 6144, "JPEG", {"quality": 90, "subsampling": 2}),
    ("camera_108mp", 12000, 9000, "JPEG", {"quality": 88, "subsampling": 2}),
    ("camera_50mp_progressive", 8192, 6144, "JPEG", {"quality": 88, "subsampling": 2, "progressive": True}),
    ("panorama", 16000, 2600, "JPEG", {"quality": 90, "subsampling": 0}),
    ("scan_a3", 9921, 7016, "PNG", {"compress_level": 1}),
    ("scan_a3_b", 9921, 7016, "PNG", {"compress_level": 1}),
    ("strip", 1600, 16000, "PNG", {"compress_level": 1}),
)
PAIRS = ((0, 1), (0, 2), (2, 3), (1, 4), (5, 6), (6, 7), (0, 5))


def picture(rng, w: int, h: int, flat: bool) -> Image.Image:
    """A small random image enlarged, so that making 100-megapixel files stays cheap: smooth with some grain for the camera
    files, flat areas for the PNG scans (the PNG decoder walks a deflate stream on one lane; a scan's stream is short)."""
    base = Image.fromarray(rng.integers(0, 256, (max(2, h // 256), max(2, w // 256), 3), dtype=np.uint8))
    if flat:
        return base.resize((w, h), Image.Resampling.NEAREST)
    big = np.asarray(base.resize((w, h), Image.Resampling.BICUBIC))
    grain = rng.integers(0, 9, (h, w, 1), dtype=np.uint8)
    return Image.fromarray(np.minimum(big, 247) + grain)


TRACED = 3                     # the files of --trace: FILES[:TRACED], and the pairs among them


def trace(K, paths, io_workers: int) -> None:
    from kobato_eyes_amd.image_io import safe_load_image

    names = ", ".join(f[0] for f in FILES[:TRACED])
    pairs = [(a, b, paths[a], paths[b]) for a, b in PAIRS if a < TRACED and b < TRACED]
    K.refine_pairs(pairs, io_workers=io_workers)                            # warm-up
    os.environ["KE_TRACE"] = "1"
    for variable in ("0", "1", "0", "1"):
        os.environ["KE_GPU_REFINE_OVERSIZE"] = variable
        with tempfile.TemporaryFile() as log:                               # the library writes its laps to the C stderr
            sys.stderr.flush()
            kept = os.dup(2)
            os.dup2(log.fileno(), 2)
            try:
                t0 = time.perf_counter()
                K.refine_pairs(pairs, io_workers=io_workers)
                seconds = time.perf_counter() - t0
            finally:
                os.dup2(kept, 2)
                os.close(kept)
            log.seek(0)
            waits = [float(x) for x in re.findall(r"\[ke_jpeg_decode\] wait for the stream\s+([0-9.]+) ms", log.read().decode(errors="replace"))]
        print(json.dumps({"bench": "refine_pairs_oversize_trace", "files": names, "pairs": len(pairs), "KE_GPU_REFINE_OVERSIZE": variable,
                          "call_seconds": round(seconds, 2), "jpeg_decode_wait_for_the_stream_ms": round(sum(waits), 2)}), flush=True)
    del os.environ["KE_TRACE"]
    t0 = time.perf_counter()
    for p in paths[:TRACED]:
        assert safe_load_image(p) is not None
    print(json.dumps({"bench": "safe_load_image_alone_one_thread", "files": names, "seconds": round(time.perf_counter() - t0, 2)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--io-workers", type=int, default=8)
    ap.add_argument("--trace", action="store_true", help="where the time of a call on the first three files goes, instead of the medians")
    args = ap.parse_args()
    import kobato_eyes_amd as K

    Image.MAX_IMAGE_PIXELS = None
    rng = np.random.default_rng(9)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for name, w, h, fmt, options in FILES[:TRACED] if args.trace else FILES:
            p = os.path.join(tmp, name + (".jpg" if fmt == "JPEG" else ".png"))
            b = io.BytesIO()
            picture(rng, w, h, flat=fmt == "PNG").save(b, fmt, **options)
            with open(p, "wb") as f:
                f.write(b.getvalue())
            paths.append(p)
            print(json.dumps({"bench": "file", "name": name, "width": w, "height": h, "format": fmt, "bytes": len(b.getvalue())}), flush=True)
        if args.trace:
            trace(K, paths, args.io_workers)
            return
        pairs = [(a, b, paths[a], paths[b]) for a, b in PAIRS]
        answers = {}
        for variable in ("0", "1"):
            os.environ["KE_GPU_REFINE_OVERSIZE"] = variable
            stats: dict = {}
            answers[variable] = K.refine_pairs(pairs, io_workers=args.io_workers, stats=stats)      # warm-up: buffers grown, code loaded
            wall = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                K.refine_pairs(pairs, io_workers=args.io_workers)
                wall.append(time.perf_counter() - t0)
            print(json.dumps({"bench": "refine_pairs_oversize", "KE_GPU_REFINE_OVERSIZE": variable, "files": len(paths), "pairs": len(pairs),
                              "io_workers": args.io_workers, "seconds_median": round(float(np.median(wall)), 3),
                              "seconds_min": round(min(wall), 3), "seconds_max": round(max(wall), 3), "repeats": args.repeats,
                              "gpu_oversize": stats.get("gpu_oversize", 0), "gpu_decodes": stats["gpu_decodes"]}), flush=True)
        assert answers["0"] == answers["1"], "the two routes disagree"
        assert all(m is not None and m.ssim is not None for m in answers["1"])


if __name__ == "__main__":
    main()
