"""ke_webpn_decode throughput: files/s at several batch sizes for animated WebP files whose frame 0 is each of the three codecs
(lossy, lossy with an alpha plane, lossless) -- 512 x 512 content as 2-frame and 16-frame animations, and a 128 x 128 frame on a
512 x 512 canvas -- against two things on the same files in the same run: the still decoder of the codec on frame 0 re-wrapped as
a still file (the ratio is what the container walk, the later frames' upload and the canvas kernel cost), and Pillow in one
process.  Then the batch hasher on files on disk with KE_GPU_WEBP_ANIMATED set and unset.  Medians of ``--repeats`` runs with the
lowest and highest.  One JSON line per measurement.

    python benchmarks/bench_webpn.py [--sizes 4096,16384] [--repeats 5] [--distinct 16] [--seam-files 2048]
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

CONTENTS = (("512_2_frames", 512, 512, 2), ("512_16_frames", 512, 512, 16), ("128_on_512_2_frames", 128, 512, 2))
STILL = {"lossy": "webp", "lossy_alpha": "webpa", "lossless": "webpl"}


def files(codec: str, side: int, canvas: int, frames: int, distinct: int) -> list:
    """[(the animation, its frame 0 re-wrapped as a still file)]"""
    import _webp_cases as W
    import _webpn_cases as N

    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:side, 0:side]
    out = []
    for k in range(distinct):
        stills = []
        for j in range(frames):
            rgb = (W.content(rng, side, side, "smooth").astype(np.int16) + rng.integers(-5, 6, (side, side, 3))).clip(0, 255).astype(np.uint8)
            buf = io.BytesIO()
            if codec == "lossy":
                Image.fromarray(rgb).save(buf, "WEBP", quality=85, method=4)
            elif codec == "lossy_alpha":
                alpha = ((np.sin((xx + 7 * k + j) / 40.0) + np.cos(yy / 31.0) + 2) * 63).astype(np.uint8)
                Image.fromarray(np.dstack([rgb, alpha]), "RGBA").save(buf, "WEBP", quality=85, method=4)
            else:
                Image.fromarray(W.content(rng, side, side, "drawing")).save(buf, "WEBP", lossless=True, quality=70, method=3)
            stills.append(N.Frame(buf.getvalue()))
        at = (canvas - side) // 2 & ~1
        data = N.animation((canvas, canvas), N.ANIMATION | (N.ALPHA if codec == "lossy_alpha" else 0),
                           [N.anim(), *(f.at(at, at) for f in stills)])
        out.append((data, stills[0].still(codec == "lossy_alpha")))
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
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--seam-files", type=int, default=2048)
    ap.add_argument("--codecs", default="lossy,lossy_alpha,lossless")
    ap.add_argument("--contents", default=",".join(c[0] for c in CONTENTS))
    args = ap.parse_args()
    import kobato_eyes_amd  # noqa: F401
    from kobato_eyes_amd import _native, fastsig

    ctx = _native.get_context(0)
    for content, side, canvas, frames in CONTENTS:
        if content not in args.contents.split(","):
            continue
        for codec in args.codecs.split(","):
            base = files(codec, side, canvas, frames, args.distinct)
            t0 = time.perf_counter()
            for a, _ in base:
                with Image.open(io.BytesIO(a)) as im:
                    im.load()
            pillow = len(base) / (time.perf_counter() - t0)
            print(json.dumps({"bench": "pillow_one_process", "content": content, "codec": codec, "files_per_s": round(pillow, 1),
                              "mean_file_bytes": int(np.mean([len(a) for a, _ in base])),
                              "mean_frame_0_bytes": int(np.mean([len(b) for _, b in base]))}), flush=True)
            for n in (int(s) for s in args.sizes.split(",")):
                animated = [base[k % len(base)][0] for k in range(n)]
                frame_0 = [base[k % len(base)][1] for k in range(n)]
                still = getattr(ctx, f"{STILL[codec]}_hash")
                for name, blobs, call in (("webpn_hash", animated, ctx.webpn_hash), (f"{STILL[codec]}_hash_frame_0_as_a_still_file", frame_0, still)):
                    call(blobs[:256])                                    # warm-up: buffers grown, code loaded
                    kernel = []

                    def once():
                        ctx.decode_kernel_ms = 0.0
                        assert not np.asarray(call(blobs)[2]).any()      # noqa: B023
                        kernel.append(ctx.decode_kernel_ms)              # noqa: B023

                    r = rate(once, n, args.repeats)
                    print(json.dumps({"bench": name, "content": content, "codec": codec, "files": n, **r,
                                      "decode_kernels_ms_median": round(float(np.median(kernel)), 2)}), flush=True)
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
                    os.environ["KE_GPU_WEBP_ANIMATED"] = variable
                    fill = lambda: rows.__setitem__(variable, fastsig.fast_fill_missing_signatures("", items, apply_to_db=False))      # noqa: E731,B023
                    fill()                                               # warm-up: worker processes started, buffers grown
                    r = rate(fill, n, args.repeats)
                    print(json.dumps({"bench": "fast_fill_missing_signatures", "KE_GPU_WEBP_ANIMATED": variable, "content": content, "codec": codec,
                                      "files": n, **r}), flush=True)
                assert rows["0"] == rows["1"] and len(rows["1"]) == n


if __name__ == "__main__":
    main()
