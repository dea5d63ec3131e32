#!/usr/bin/env python3
"""Wall time of the decode + hash call under two builds of the library, in turns on one box: for a change that should leave the
host side of ke_jpeg_decode / ke_png_decode as fast as it was.

    python benchmarks/bench_decode_builds.py --other /path/to/the/other/libkeyes_hip.so [--turns 5] [ROW ...]

rows (the file sets of benchmarks/bench_jpeg.py and benchmarks/bench_jpeg_restarts.py):
    jpeg_default        bench_jpeg.py                               16 384 files of 512 x 512
    jpeg_65536x128      bench_jpeg.py --images 65536 --side 128     the most host work per kernel time
    jpeg_progressive    bench_jpeg.py --progressive
    png                 bench_jpeg.py --format png
    restarts_128_unset  bench_jpeg_restarts.py --rows 12mp_rows1, 128 files per call, KE_JPEG_SPLIT_RESTARTS unset
    restarts_128_set    the same files, KE_JPEG_SPLIT_RESTARTS=1

A measurement is a fresh process with KE_LIBKEYES naming the build: a warm-up call on the whole batch, then 3 timed
``Context.jpeg_hash`` calls, their median.  ``--turns`` such processes per build and row, the two builds alternating.  One JSON
line per row: per build the median, lowest and highest of the turns.  The margin to hold a difference against is the spread of
the other build's own turns.  The two builds must return the same hashes."""
from __future__ import annotations

import argparse
import io
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROWS = {   # name: (kind, files per call, side, progressive, environment)
    "jpeg_default": ("jpeg", 16384, 512, False, {}),
    "jpeg_65536x128": ("jpeg", 65536, 128, False, {}),
    "jpeg_progressive": ("jpeg", 16384, 512, True, {}),
    "png": ("png", 16384, 512, False, {}),
    "restarts_128_unset": ("restarts", 128, 0, False, {}),
    "restarts_128_set": ("restarts", 128, 0, False, {"KE_JPEG_SPLIT_RESTARTS": "1"}),
}


def measure(path: str) -> None:
    from kobato_eyes_amd import _native

    kind, n, files = pickle.load(open(path, "rb"))
    blobs = [files[k % len(files)] for k in range(n)]
    fmt = "png" if kind == "png" else "jpeg"
    ctx = _native.Context(0)
    ctx.jpeg_hash(blobs[:512], kind=fmt)
    ph, _, st = ctx.jpeg_hash(blobs, want_dhash=False, kind=fmt)
    assert (st == 0).all()
    wall, kern = [], []
    for _ in range(3):
        t0, k0 = time.perf_counter(), ctx.decode_kernel_ms
        ph2, _, st = ctx.jpeg_hash(blobs, want_dhash=False, kind=fmt)
        wall.append(time.perf_counter() - t0)
        kern.append(ctx.decode_kernel_ms - k0)
    assert np.array_equal(ph, ph2)
    print("RESULT " + json.dumps({"wall_ms": float(np.median(wall)) * 1e3, "kernel_ms": float(np.median(kern)), "hash_crc": zlib.crc32(ph.tobytes())}))


def make_files(path: str, kind: str, n: int, side: int, progressive: bool) -> None:
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    if kind == "restarts":
        import bench_jpeg_restarts as R

        w, h, options, _, distinct = R.ROWS["12mp_rows1"]
        rng = np.random.default_rng([12, w, h])
        pictures = [R.picture(rng, w, h) for _ in range(distinct)]
        save = {"format": "JPEG", "quality": 85, "subsampling": 2, **options}
    else:
        from kobato_eyes_amd import _native

        pictures = [Image.fromarray(a) for a in _native.Context(0).synth_rgb(20260604, 0, 4096, side, side)]
        save = {"format": "PNG"} if kind == "png" else {"format": "JPEG", "quality": 85, "subsampling": 2, "progressive": progressive}

    def encode(im):
        b = io.BytesIO()
        im.save(b, **save)
        return b.getvalue()

    with ThreadPoolExecutor(16) as ex:
        pickle.dump((kind, n, list(ex.map(encode, pictures))), open(path, "wb"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the library to compare this tree's against (KE_LIBKEYES)")
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("rows", nargs="*", default=list(ROWS))
    args = ap.parse_args()
    builds = {"other": os.path.abspath(args.other), "this": os.path.join(ROOT, "kobato-eyes_amd", "libkeyes_hip.so")}
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as tmp:
        for row in args.rows:
            kind, n, side, progressive, env = ROWS[row]
            path = os.path.join(tmp, f"{kind}_{side}_{int(progressive)}.pkl")
            if not os.path.exists(path):                     # (a process of its own: this one never opens the GPU)
                subprocess.run([sys.executable, me, "--make", path, kind, str(n), str(side), str(int(progressive))], check=True, timeout=900)
            results = {"other": [], "this": []}
            for _ in range(args.turns):
                for build in ("other", "this"):
                    out = subprocess.run([sys.executable, me, "--measure", path], env=dict(os.environ, KE_LIBKEYES=builds[build], **env),
                                         capture_output=True, text=True, timeout=600)
                    if out.returncode != 0:                  # trouble ends the run: nothing more is started on the GPU
                        sys.exit(f"{row} / {build}: exit {out.returncode}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
                    results[build].append(json.loads([line for line in out.stdout.splitlines() if line.startswith("RESULT ")][0][7:]))
            assert len({r["hash_crc"] for rs in results.values() for r in rs}) == 1, "the builds disagree"
            line = {"bench": "decode_hash_two_builds", "row": row, "files_per_call": n, "env": env, "turns": args.turns}
            for build, rs in results.items():
                wall = [r["wall_ms"] for r in rs]
                line[build] = {"wall_ms_median": round(float(np.median(wall)), 2), "wall_ms_lowest": round(min(wall), 2), "wall_ms_highest": round(max(wall), 2),
                               "kernel_ms_median": round(float(np.median([r["kernel_ms"] for r in rs])), 2)}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--measure":
        measure(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "--make":
        make_files(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), bool(int(sys.argv[6])))
    else:
        main()
