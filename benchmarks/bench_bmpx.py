"""ke_bmpx_decode throughput: decode + hash files/s at several batch sizes for 512 x 512 BMP files -- RLE8 drawing-like and
photograph-like (through the greedy encoder of tests/_bmpx_write.py), RLE4 drawing-like, uncompressed 4-bit, 1-bit and 16-bit, the
files repeated from a few distinct ones -- against the yardsticks taken in the same run on the same pixels: ke_bmp_decode on the
8-bit uncompressed form of every palette config, Pillow in one process, and the batch hasher over files on disk with
KE_GPU_BMP_EXTENDED unset against set (after one pass each way that is not counted).  Median of --repeats with lowest and highest everywhere but for Pillow in one
process (one pass over the distinct files).  With each rate the decode kernels' time (ke_last_kernel_ms) and, for the kinds
ke_bmpx_unpack alone decodes, the bytes it reads and writes per second of that time.  One JSON line per measurement.

    python benchmarks/bench_bmpx.py [--sizes 4096,16384] [--repeats 5] [--distinct 32] [--seam-files 2048] [--out FILE]

Not measured here: 65 536 files per call, files larger than 512 x 512.
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

import _bmpx_cases as X  # noqa: E402
import _bmpx_write as Wr  # noqa: E402
from bench_tiffc import images  # noqa: E402

# (config, content, kind, colours)
CONFIGS = [("rle8", "drawing", "rle8", 256), ("rle8", "photo", "rle8", 256), ("rle4", "drawing", "rle4", 16), ("p4", "photo", "p4", 16),
           ("p1", "photo", "p1", 2), ("rgb565", "photo", "rgb565", 0)]


def quantised(a: np.ndarray, n: int):
    """(indices, palette as B G R X bytes) of Pillow's quantiser; entry 0 never black, so that the file is a palette file."""
    q = Image.fromarray(a).quantize(n)
    pal = np.asarray(q.getpalette()[:3 * n], np.uint8).reshape(-1, 3)
    pal = np.concatenate([pal[:, ::-1], np.zeros((len(pal), 1), np.uint8)], 1)
    if not pal[0, :3].any():
        pal[0, :3] = (1, 1, 1)
    return np.asarray(q), pal.tobytes()


def written(a: np.ndarray, kind: str, n: int) -> bytes:
    if kind == "rgb565":
        p = a.astype(np.uint16)
        return X.picture(kind, (p[..., 0] >> 3 << 11) | (p[..., 1] >> 2 << 5) | (p[..., 2] >> 3))
    idx, pal = quantised(a, n)
    if kind == "bmp8":                                           # the same pixels as ke_bmp_decode takes them (it leaves two colours to Pillow: 256 entries)
        return Wr.bmp(idx.shape[1], idx.shape[0], 8, Wr._stored(idx, False), colors=256, palette=pal + bytes(4 * (256 - n)))
    return X.picture(kind, idx, pal=pal)


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

    def rate(bench: str, kind: str, config: str, hash_call, base: list, pixel_bytes: int = 0) -> None:
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
            row = {"bench": bench, "kind": kind, "config": config, "files": n, "repeats": args.repeats,
                   "files_per_s_median": round(n / float(np.median(wall)), 1), "files_per_s_lowest": round(n / max(wall), 1),
                   "files_per_s_highest": round(n / min(wall), 1), "decode_kernels_ms_median": round(float(np.median(kernel)), 2),
                   "mean_file_bytes": int(np.mean([len(d) for d in base]))}
            if pixel_bytes:                                      # ke_bmpx_unpack alone: bytes in + bytes out over the kernels' time
                moved = n * (row["mean_file_bytes"] + pixel_bytes)
                row["unpack_gb_per_s_of_kernel_time"] = round(moved / (float(np.median(kernel)) * 1e-3) / 1e9, 1)
            report(row)

    pixels = {kind: images(kind, args.distinct) for kind in ("photo", "drawing")}
    for config, kind, fmt, colours in CONFIGS:
        base = [written(a, fmt, colours) for a in pixels[kind]]
        if fmt != "rgb565":                                      # (a 16-bit file has no 8-bit form)
            rate("bmp_hash_8bit_uncompressed", kind, f"{config}_pixels", ctx.bmp_hash, [written(a, "bmp8", colours) for a in pixels[kind]])
        t0 = time.perf_counter()
        for d in base:
            with Image.open(io.BytesIO(d)) as im:
                im.load()
        report({"bench": "pillow_one_process", "kind": kind, "config": config, "files_per_s": round(len(base) / (time.perf_counter() - t0), 1),
                "mean_file_bytes": int(np.mean([len(d) for d in base]))})
        rate("bmpx_hash", kind, config, ctx.bmpx_hash, base, 0 if fmt in ("rle8", "rle4") else 512 * 512 * (3 if fmt == "rgb565" else 1))
        if args.seam_files <= 0:
            continue
        with tempfile.TemporaryDirectory() as tmp:               # the batch hasher over files on disk, the variable unset and set
            items = []
            for k in range(args.seam_files):
                p = os.path.join(tmp, f"{k:05d}.bmp")
                with open(p, "wb") as f:
                    f.write(base[k % len(base)])
                items.append((k, p))
            rows = {}
            # one pass each way that is not counted (it also starts the decoder processes), then --repeats each way, alternating
            for k, setting in enumerate(("0", "1") * (1 + args.repeats)):
                os.environ["KE_GPU_BMP_EXTENDED"] = setting
                t0 = time.perf_counter()
                got = K.compute_signatures_mp(items)
                took = time.perf_counter() - t0
                assert len(got) == len(items) and rows.setdefault("rows", got) == got
                if k >= 2:
                    rows.setdefault(setting, []).append(took)
            os.environ.pop("KE_GPU_BMP_EXTENDED", None)
            row = {"bench": "batch_hasher_seam", "kind": kind, "config": config, "files": len(items), "repeats": args.repeats}
            for setting, label in (("0", "unset"), ("1", "set")):
                row.update({f"files_per_s_variable_{label}_median": round(len(items) / float(np.median(rows[setting])), 1),
                            f"files_per_s_variable_{label}_lowest": round(len(items) / max(rows[setting]), 1),
                            f"files_per_s_variable_{label}_highest": round(len(items) / min(rows[setting]), 1)})
            report(row)


if __name__ == "__main__":
    main()
