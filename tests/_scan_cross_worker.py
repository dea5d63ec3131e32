"""Child process of tests/test_gpu_turned.py: every table of tests/_scan_from_cases.py through ke_hamming_scan_cross under the
KE_SCAN_MODE of this process's environment (the library reads it once), beside the full scan of the same table.
python _scan_cross_worker.py ROOT OUT.npz"""
import ctypes as C
import os
import sys

ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import _scan_from_cases as S
from kobato_eyes_amd import _native

ctx = _native.Context(0)
MODE = os.environ.get("KE_SCAN_MODE", "auto")


def rows(e):
    r = np.stack([e["a"].astype(np.int64), e["b"].astype(np.int64), e["h"].astype(np.int64), e["bands"].astype(np.int64)], axis=1)
    return r[np.lexsort(r.T[::-1])]


def scan(c, first_new, part_index=0, part_count=1):
    """first_new None: ke_hamming_scan of the whole table, else ke_hamming_scan_cross."""
    kw = dict(ids=c["ids"], sizes=c["sizes"], part_index=part_index, part_count=part_count, **c["kw"])
    if first_new is None:
        e, cnt = ctx.hamming_scan(c["h"], len(c["h"]), **kw)
    else:
        e, cnt = ctx.hamming_scan(c["h"], len(c["h"]), first_new=first_new, cross=True, **kw)
    return rows(e), cnt.astype(np.uint64), ctx.last_scan_path()


def raw_cross(c, first_new, edges, capacity, counters):
    addr = lambda a: None if a is None else a.ctypes.data
    n_edges, k = C.c_int64(0), c["kw"]
    rc = ctx._lib.ke_hamming_scan_cross(ctx._h, c["h"].ctypes.data, addr(c["ids"]), addr(c["sizes"]), len(c["h"]), first_new, 0, 1,
                                        k["threshold"], k["band_bits"], k["band_count"], float(k["size_ratio"]),
                                        int(k["bucket_pair_cap"]), addr(edges), capacity, C.byref(n_edges), addr(counters))
    return rc, n_edges.value


out = {}
cases = S.small_cases()
for name, c in cases.items():
    out[f"{name}/full/edges"], out[f"{name}/full/counters"], _ = scan(c, None)
    for f in S.FIRST_NEW:
        out[f"{name}/{f}/edges"], out[f"{name}/{f}/counters"], path = scan(c, f)
        out[f"{name}/{f}/path"] = np.array(path, np.int64)

c = cases["plain"]
for f in S.SHARD_FIRST_NEW:
    for parts in S.PARTS:
        got = [scan(c, f, p, parts) for p in range(parts)]
        out[f"shards/{f}/{parts}/edges"] = np.concatenate([g[0] for g in got])     # a pair found twice stays twice
        out[f"shards/{f}/{parts}/counters"] = np.stack([g[1] for g in got])
        out[f"shards/{f}/{parts}/paths"] = np.array([g[2] for g in got], np.int64)

# one raw call with a buffer of four edges: the count it reports is the region's whole edge count
buf, cnt = np.zeros(S.SMALL_CAPACITY, _native.EDGE_DTYPE), np.zeros(4, np.uint64)
rc, reported = raw_cross(c, 1025, buf, S.SMALL_CAPACITY, cnt)
ctx._check(rc, "ke_hamming_scan_cross")
out["small-capacity/reported"] = np.array([reported, int(cnt[2])], np.int64)
out["small-capacity/stored"] = rows(buf)
# ... and the binding's overflow protocol from there to the whole list
e, _ = ctx.hamming_scan(c["h"], S.N, first_new=1025, cross=True, capacity=S.SMALL_CAPACITY, **c["kw"])
out["small-capacity/grown"] = rows(e)
# first_new outside [0, n] is refused without a launch
out["einval"] = np.array([raw_cross(c, bad, None, 0, None)[0] for bad in (-1, S.N + 1)], np.int64)

if MODE == "auto":
    big = S.big_case()
    out["big/full/edges"], out["big/full/counters"], _ = scan(big, None)
    out["big/cross/edges"], out["big/cross/counters"], path = scan(big, S.BIG_FIRST_NEW_WIDE)
    out["big/cross/path"] = np.array(path, np.int64)
    print(f"big case, first_new = {S.BIG_FIRST_NEW_WIDE}: auto took path {path} (0 tiles, 1 buckets)")

np.savez(OUT, mode=np.array(MODE), **out)
