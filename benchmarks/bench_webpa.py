"""ke_webpa_decode throughput: files/s at several batch sizes for 512 x 512 lossy WebP files (quality 85) with three kinds of
alpha plane -- a cut-out mask (compresses to a few hundred bytes), a smooth gradient, and noise (which libwebp stores raw) --
against two things on the same files in the same run: Pillow (one process, and the batch hasher's Pillow route), and
ke_webp_decode on the same "VP8 " payloads without the plane.  The ratio to the latter is what the plane costs.  One JSON
line per measurement.

    python benchmarks/bench_webpa.py [--sizes 4096,16384] [--repeats 5] [--distinct 32] [--seam-files 4096]
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


def files(kind: str, distinct: int, side: int = 512) -> list:
    """[(file with the plane, the same frame as a plain lossy file)]"""
    import _webp_cases as W

    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:side, 0:side]
    out = []
    for k in range(distinct):
        rgb = (W.content(rng, side, side, "smooth").astype(np.int16) + rng.integers(-5, 6, (side, side, 3))).clip(0, 255).astype(np.uint8)
        if kind == "mask":
            cx, cy, r = side / 2 + 3 * k, side / 2 - 2 * k, side / 3 + k
            alpha = np.where((xx - cx) ** 2 + (yy - cy) ** 2 < r * r, 255, 0).astype(np.uint8)
        elif kind == "smooth":
            alpha = ((np.sin((xx + 7 * k) / 40.0) + np.cos(yy / 31.0) + 2) * 63).astype(np.uint8)
        else:
            alpha = rng.integers(0, 256, (side, side), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(np.dstack([rgb, alpha]), "RGBA").save(buf, "WEBP", quality=85, method=4)
        data = buf.getvalue()
        out.append((data, W.riff([(b"VP8 ", W.vp8_of(data))])))
    return out


def rate(fn, n: int, repeats: int):
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
    return {"files_per_s_median": round(n / float(np.median(wall)), 1), "files_per_s_min": round(n / max(wall), 1),
            "files_per_s_max": round(n / min(wall), 1), "repeats": repeats}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--seam-files", type=int, default=4096)
    args = ap.parse_args()
    import _webp_cases as W
    import kobato_eyes_amd  # noqa: F401
    from kobato_eyes_amd import _native, fastsig

    ctx = _native.get_context(0)
    for kind in ("mask", "smooth", "noise"):
        base = files(kind, args.distinct)
        header = sorted({next(p for t, p in W.chunks(a) if t == b"ALPH")[0] for a, _ in base})
        t0 = time.perf_counter()
        for a, _ in base:
            with Image.open(io.BytesIO(a)) as im:
                im.load()
        pillow = len(base) / (time.perf_counter() - t0)
        print(json.dumps({"bench": "pillow_one_process", "kind": kind, "files_per_s": round(pillow, 1), "alph_header_bytes": header,
                          "mean_file_bytes": int(np.mean([len(a) for a, _ in base])),
                          "mean_alph_bytes": int(np.mean([len(a) - len(b) for a, b in base]))}), flush=True)
        for n in (int(s) for s in args.sizes.split(",")):
            with_plane = [base[k % len(base)][0] for k in range(n)]
            frame_only = [base[k % len(base)][1] for k in range(n)]
            for name, blobs, call in (("webpa_hash", with_plane, ctx.webpa_hash), ("webp_hash_same_frames", frame_only, ctx.webp_hash)):
                call(blobs[:256])                                    # warm-up: buffers grown, code loaded
                kernel = []

                def once():
                    ctx.decode_kernel_ms = 0.0
                    assert not np.asarray(call(blobs)[2]).any()
                    kernel.append(ctx.decode_kernel_ms)

                r = rate(once, n, args.repeats)
                print(json.dumps({"bench": name, "kind": kind, "files": n, **r, "decode_kernels_ms_median": round(float(np.median(kernel)), 2)}), flush=True)
        # the batch hasher on files on disk: the Pillow route (variable unset) and the GPU route
        n = args.seam_files
        with tempfile.TemporaryDirectory() as tmp:
            items = []
            for k in range(n):
                p = os.path.join(tmp, f"{k:05d}.webp")
                with open(p, "wb") as f:
                    f.write(base[k % len(base)][0])
                items.append((k, p))
            rows = {}
            for variable in ("0", "1"):
                os.environ["KE_GPU_WEBP_ALPHA"] = variable
                fill = lambda: rows.__setitem__(variable, fastsig.fast_fill_missing_signatures("", items, apply_to_db=False))      # noqa: E731,B023
                fill()                                               # warm-up: worker processes started, buffers grown
                r = rate(fill, n, max(2, args.repeats // 2))
                print(json.dumps({"bench": "fast_fill_missing_signatures", "KE_GPU_WEBP_ALPHA": variable, "kind": kind, "files": n, **r}), flush=True)
            assert rows["0"] == rows["1"] and len(rows["1"]) == n


if __name__ == "__main__":
    main()
