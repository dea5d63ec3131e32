"""Child process of tests/test_gpu_scan_from.py: every table of tests/_scan_from_cases.py through ke_hamming_scan_from under
the KE_SCAN_MODE of this process's environment (the library reads it once), beside the full scan of the same table.
python _scan_from_worker.py ROOT OUT.npz"""
import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import _scan_from_cases as S
from kobato_eyes_amd import _native
from kobato_eyes_amd.scanner import DuplicateFile, DuplicateScanConfig, DuplicateScanner

ctx = _native.Context(0)


def rows(e):
    r = np.stack([e["a"].astype(np.int64), e["b"].astype(np.int64), e["h"].astype(np.int64), e["bands"].astype(np.int64)], axis=1)
    return r[np.lexsort(r.T[::-1])]


def scan(c, first_new, part_index=0, part_count=1):
    """first_new None: the existing entry.  0: the new entry called directly (the binding sends 0 to the existing one)."""
    kw = dict(ids=c["ids"], sizes=c["sizes"], part_index=part_index, part_count=part_count, **c["kw"])
    if first_new != 0:
        e, cnt = ctx.hamming_scan(c["h"], len(c["h"]), **({} if first_new is None else {"first_new": first_new}), **kw)
    else:
        addr = lambda a: None if a is None else a.ctypes.data
        e, cnt, n_edges = np.zeros(1 << 16, _native.EDGE_DTYPE), np.zeros(4, np.uint64), C.c_int64(0)
        k = c["kw"]
        rc = ctx._lib.ke_hamming_scan_from(ctx._h, c["h"].ctypes.data, addr(c["ids"]), addr(c["sizes"]), len(c["h"]), 0, part_index,
                                           part_count, k["threshold"], k["band_bits"], k["band_count"], float(k["size_ratio"]),
                                           int(k["bucket_pair_cap"]), e.ctypes.data, len(e), C.byref(n_edges), cnt.ctypes.data)
        ctx._check(rc, "ke_hamming_scan_from")
        assert n_edges.value <= len(e)
        e = e[: n_edges.value]
    return rows(e), cnt.astype(np.uint64), ctx.last_scan_path()


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
buf = np.zeros(S.SMALL_CAPACITY, _native.EDGE_DTYPE)
n_edges, cnt = C.c_int64(0), np.zeros(4, np.uint64)
kw = c["kw"]
rc = ctx._lib.ke_hamming_scan_from(ctx._h, c["h"].ctypes.data, None, None, S.N, 1025, 0, 1, kw["threshold"], kw["band_bits"],
                                   kw["band_count"], float(kw["size_ratio"]), int(kw["bucket_pair_cap"]), buf.ctypes.data,
                                   S.SMALL_CAPACITY, C.byref(n_edges), cnt.ctypes.data)
ctx._check(rc, "ke_hamming_scan_from")
out["small-capacity/reported"] = np.array([n_edges.value, int(cnt[2])], np.int64)
out["small-capacity/stored"] = rows(buf)
# first_new outside [0, n] is refused without a launch
out["einval"] = np.array([ctx._lib.ke_hamming_scan_from(ctx._h, c["h"].ctypes.data, None, None, S.N, bad, 0, 1, 8, 16, 4, 0.0, 0, None, 0,
                                                        C.byref(n_edges), None) for bad in (-1, S.N + 1)], np.int64)

big = S.big_case()
out["big/full/edges"], out["big/full/counters"], _ = scan(big, None)
out["big/from/edges"], out["big/from/counters"], path = scan(big, S.BIG_FIRST_NEW)
out["big/from/path"] = np.array(path, np.int64)
out["big/wide/edges"], out["big/wide/counters"], path = scan(big, S.BIG_FIRST_NEW_WIDE)
out["big/wide/path"] = np.array(path, np.int64)


# extend_clusters against build_clusters of the whole on the 2 500 table
def flat(clusters):
    return [[cl.keeper_id, [[e.file.file_id, e.best_hamming] for e in cl.files]] for cl in clusters]


files = [DuplicateFile(i, Path(p), s, w, h_, ph) for i, p, s, w, h_, ph in S.cluster_files()]
scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=S.THRESHOLD))
library, added = files[:S.CLUSTER_SPLIT], files[S.CLUSTER_SPLIT:]
previous = scanner.build_clusters(library)
clusters = {"whole": flat(scanner.build_clusters(files)), "previous": flat(previous),
            "extended": flat(scanner.extend_clusters(library, added, previous))}
np.savez(OUT, mode=np.array(os.environ.get("KE_SCAN_MODE", "auto")), clusters=np.array(json.dumps(clusters)), **out)
