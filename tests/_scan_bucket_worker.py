"""Child process of tests/test_gpu_scan_buckets.py: every case of tests/_scan_bucket_cases.py under the KE_SCAN_MODE of
this process's environment (the library reads it once).  python _scan_bucket_worker.py ROOT OUT.npz"""
import ctypes as C
import os
import sys

ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import _scan_bucket_cases as S
from kobato_eyes_amd import _native

ctx = _native.Context(0)


def rows(e):
    r = np.stack([e["a"].astype(np.int64), e["b"].astype(np.int64), e["h"].astype(np.int64), e["bands"].astype(np.int64)], axis=1)
    return r[np.lexsort(r.T[::-1])]


out = {}
for name, c in S.cases().items():
    h, n = c["h"], len(c["h"])
    for parts in c["parts"]:
        edges, counters, paths = [], [], []
        for p in range(parts):
            e, cnt = ctx.hamming_scan(h, n, ids=c["ids"], sizes=c["sizes"], part_index=p, part_count=parts, capacity=c["capacity"], **c["kw"])
            edges.append(rows(e))
            counters.append(cnt.astype(np.uint64))
            paths.append(ctx.last_scan_path())
        tag = f"{name}/{parts}"
        out[tag + "/edges"] = np.concatenate(edges)                # shard after shard: a pair found twice stays twice
        out[tag + "/counters"] = np.stack(counters)
        out[tag + "/paths"] = np.array(paths, np.int64)
    if c["capacity"]:
        # one raw call with the small buffer: the count it reports is the whole edge count, and only `capacity` edges are stored
        buf = np.zeros(c["capacity"], _native.EDGE_DTYPE)
        n_edges, cnt = C.c_int64(0), np.zeros(4, np.uint64)
        kw = c["kw"]
        rc = ctx._lib.ke_hamming_scan(ctx._h, h.ctypes.data, None, None, n, 0, 1, kw["threshold"], kw["band_bits"], kw["band_count"],
                                      float(kw["size_ratio"]), int(kw["bucket_pair_cap"]), buf.ctypes.data, c["capacity"],
                                      C.byref(n_edges), cnt.ctypes.data)
        ctx._check(rc, "ke_hamming_scan")
        out[name + "/reported"] = np.array([n_edges.value, int(cnt[2])], np.int64)
        out[name + "/stored"] = rows(buf)
np.savez(OUT, mode=np.array(os.environ.get("KE_SCAN_MODE", "auto")), **out)
