#!/usr/bin/env python3
"""The exact scan (ke_hamming_scan_exact) beside the banded scans of the same table: HIP-event times of everything each call
launches (ke_last_kernel_ms), on device-resident tables of ke_synth_hashes, T = 8.  One JSON line per row, appended to --out as
well (profiles/r25_scan_exact.jsonl is the record).

    python benchmarks/bench_scan_exact.py [--n N ...] [--check] [--out FILE]         # everything below, one child after the other
    python benchmarks/bench_scan_exact.py --leg tiles|auto|cross [...]                # one leg, in this process
    python benchmarks/bench_scan_exact.py --leg banded --root TREE --tag NAME         # ke_hamming_scan under KE_SCAN_MODE=tiles
                                                                                      # alone, e.g. of another build

The library reads KE_SCAN_MODE once per process, so "banded under tiles" and "banded under auto" cannot share a process.  Each
is therefore a leg -- a child process started by the plain call, one at a time, none after one that fails -- and the exact
scan is timed again in every leg, in turns with that leg's banded calls, so that each comparison is made inside one process:
  tiles : exact | ke_hamming_scan under KE_SCAN_MODE=tiles                       (the same kernel: the times should agree)
  auto  : exact | ke_hamming_scan under auto | ke_hamming_scan with band_bits=1, band_count=64 (the old route to the exact set)
  cross : exact cross scans of [100 000 | 700 000] and [1 000 000 | 7 000 000], with the launches each took
Each figure is the median of 5 timed calls after 2 untimed ones, with the lowest and the highest.  --check holds a sample of
rows to the NumPy definition in the run: for each sampled row, its partners within T by xor and np.bitwise_count over the whole
table against the edges the scan returned for that row.  One GPU; nothing here runs on more than one."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("tiles", "auto", "cross", "banded"), default=None)
ap.add_argument("--n", type=int, nargs="*", default=[100_000, 1_000_000])
ap.add_argument("--cross", type=int, nargs="*", default=[100_000, 1_000_000], help="library sizes L of the [L | 7 L] cross scans")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--check", action="store_true")
ap.add_argument("--sample", type=int, default=48, help="--check: rows held to the definition per table")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package is timed")
ap.add_argument("--tag", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.leg is None:
    passed_on = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--sample", str(args.sample), "--root", args.root]
    passed_on += ["--check"] if args.check else []
    passed_on += ["--out", args.out] if args.out else []
    for leg in ("tiles", "auto", "cross"):
        sizes = ["--cross", *map(str, args.cross)] if leg == "cross" else ["--n", *map(str, args.n)]
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, *sizes, *passed_on]).returncode
        if rc != 0:
            sys.exit(f"leg {leg} ended with {rc}: nothing further is started")
    sys.exit(0)

if args.leg in ("tiles", "banded"):
    os.environ["KE_SCAN_MODE"] = "tiles"
elif args.leg == "auto":
    os.environ.pop("KE_SCAN_MODE", None)

sys.path.insert(0, args.root)
import numpy as np  # noqa: E402

from kobato_eyes_amd import _native  # noqa: E402

SEED = 20260604
T = 8
TILE = 1024
MAX_LAUNCH = 0xFFFFFFFF // 512


def stats(ms):
    return {"median": float(np.median(ms)), "lowest": float(min(ms)), "highest": float(max(ms))}


def spread(s):
    return s["highest"] - s["lowest"]


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def launches(tiles: int) -> int:
    per = int(os.environ.get("KE_SCAN_TILES_PER_LAUNCH") or 0)
    per = per if 0 < per < MAX_LAUNCH else MAX_LAUNCH
    return -(-tiles // per)


def timed(ways: dict) -> dict:
    """{name: call} -> {name: (last result, [ms])}, the calls in turns so that all see the same neighbours."""
    got = {name: [None, []] for name in ways}
    for _ in range(args.warmup + args.reps):
        for name, call in ways.items():
            got[name][0] = call()
            got[name][1].append(ctx.last_kernel_ms(1))
    return {name: (res, stats(ms[args.warmup:])) for name, (res, ms) in got.items()}


def check(host, edges, first_new=None):
    """A sample of rows against the definition: row i's partners within T (cross: on the other side of first_new)."""
    rng = np.random.default_rng(len(host))
    n = len(host)
    a, b = edges["a"].astype(np.int64), edges["b"].astype(np.int64)
    touching = np.unique(np.concatenate([a, b]))
    rows = np.concatenate([rng.choice(touching, min(args.sample // 2, len(touching)), replace=False), rng.integers(0, n, args.sample // 2)])
    for i in rows.tolist():
        near = np.nonzero(np.bitwise_count(host ^ host[i]) <= T)[0]
        near = near[near != i]
        if first_new is not None:
            near = near[near >= first_new] if i < first_new else near[near < first_new]
        got = np.sort(np.concatenate([b[a == i], a[b == i]]))
        assert np.array_equal(got, near), f"row {i}: the scan has {got.tolist()}, the definition {near.tolist()}"
    return len(rows)


ctx = _native.Context(0)
if args.leg == "cross":
    for lib_n in args.cross:
        n = 8 * lib_n
        d = ctx.malloc(n * 8)
        ctx.synth_hashes(SEED, n, out=d)
        cap = [max(1 << 16, 2 * n)]

        def exact_cross():
            e, c = ctx.hamming_scan(d, n, threshold=T, capacity=cap[0], first_new=lib_n, cross=True, exact=True)
            cap[0] = max(cap[0], len(e))
            return e, c

        (edges, counters), ms = timed({"exact": exact_cross})["exact"]
        tiles = -(-lib_n // TILE) * (-(-n // TILE) - lib_n // TILE)
        row = {"case": "exact_cross", "library": lib_n, "queries": n - lib_n, "region_pairs": int(counters[0]), "tiles": tiles,
               "launches": launches(tiles), "edges": int(len(edges)), "bandless_edges": int((edges["bands"] == 0).sum()), "exact_ms": ms,
               "tera_pairs_per_s": int(counters[0]) / ms["median"] / 1e9, "path": ctx.last_scan_path(), "gpus": 1}
        if args.check:
            row["rows_checked"] = check(ctx.synth_hashes(SEED, n), edges, first_new=lib_n)
        emit(row)
        ctx.free(d)
    sys.exit(0)

for n in args.n:
    d = ctx.malloc(n * 8)
    ctx.synth_hashes(SEED, n, out=d)
    cap = [max(1 << 16, 2 * n)]

    def scan(**kw):
        def call():
            e, c = ctx.hamming_scan(d, n, threshold=T, capacity=cap[0], **kw)
            cap[0] = max(cap[0], len(e))
            return e, c, ctx.last_scan_path()
        return call

    if args.leg == "banded":
        (edges, counters, path), ms = timed({"banded": scan()})["banded"]
        emit({"case": "banded_only", "tag": args.tag, "n": n, "mode": "tiles", "path": path, "edges": int(len(edges)), "banded_ms": ms, "gpus": 1})
        ctx.free(d)
        continue
    ways = {"exact": scan(exact=True), "banded": scan()}
    if args.leg == "auto":
        ways["ones"] = scan(band_bits=1, band_count=64)
    got = timed(ways)
    (edges, counters, path), ms = got["exact"]
    (b_edges, b_counters, b_path), b_ms = got["banded"]
    assert len(b_edges) == int((edges["bands"] != 0).sum()), "the exact edges with a shared band are not the banded scan's"
    margin = max(spread(ms), spread(b_ms))
    row = {"case": "scan_exact", "leg": args.leg, "n": n, "pairs": int(counters[0]), "edges": int(len(edges)),
           "bandless_edges": int((edges["bands"] == 0).sum()), "banded_edges": int(len(b_edges)), "exact_path": path, "banded_path": b_path,
           "exact_ms": ms, "banded_ms": b_ms, "gpus": 1}
    if args.leg == "tiles":        # the same kernel on both sides: exact may exceed banded by at most the larger of the two spreads
        row.update({"exact_minus_banded_ms": ms["median"] - b_ms["median"], "margin_ms": margin,
                    "within_margin": bool(ms["median"] - b_ms["median"] <= margin)})
    if "ones" in got:
        (o_edges, _, o_path), o_ms = got["ones"]
        assert len(o_edges) == len(edges), "band_bits=1, band_count=64 does not give the exact edge count"
        row.update({"ones_ms": o_ms, "ones_path": o_path, "ones_over_exact": o_ms["median"] / ms["median"]})
    if args.check:
        row["rows_checked"] = check(ctx.synth_hashes(SEED, n), edges)
    emit(row)
    ctx.free(d)
