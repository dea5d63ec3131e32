"""Child process of tests/test_gpu_scan_exact.py: the exact scan of one table of 5 000 hashes (15 tiles of 1024 x 1024) in
all three regions, under the KE_SCAN_TILES_PER_LAUNCH of this process's environment (the library reads it once).
python _scan_exact_worker.py ROOT OUT.npz"""
import os
import sys

ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import _scan_exact_cases as X
from kobato_eyes_amd import _native

N, FIRST_NEW = 5000, 2100
ctx = _native.Context(0)
h, ids, sizes = X.table(N, seed=5)
out = {}
for name, region in (("all", {}), ("from", {"first_new": FIRST_NEW}), ("cross", {"first_new": FIRST_NEW, "cross": True})):
    for parts in (1, 3):
        edges, counters = [], []
        for p in range(parts):
            e, c = ctx.hamming_scan(h, N, ids=ids, sizes=sizes, threshold=X.THRESHOLD, size_ratio=0.5, part_index=p, part_count=parts,
                                    exact=True, **region)
            assert ctx.last_scan_path() == 0
            edges.append(X.edge_rows(e))
            counters.append(c.astype(np.uint64))
        out[f"{name}/{parts}/edges"] = np.concatenate(edges)          # shard after shard: a pair found twice stays twice
        out[f"{name}/{parts}/counters"] = np.stack(counters)
np.savez(OUT, per_launch=np.array(os.environ.get("KE_SCAN_TILES_PER_LAUNCH", "")), **out)
