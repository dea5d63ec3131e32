"""A stand-in for _native.Context on a machine without a GPU, shared by the tests of DuplicateScanner's view scans
(test_turned_cpu.py, test_trimmed_cpu.py, test_view_scan_cpu.py, test_gpu_trimmed.py): ``hamming_scan`` is the host oracle's
banded scan cut to the region asked for."""
from __future__ import annotations

import numpy as np

from kobato_eyes_amd._native import EDGE_DTYPE
from oracle import oracle as O


class OracleScanContext:
    """``hamming_scan`` is the oracle's banded scan filtered by b >= first_new -- what ke_hamming_scan_from is specified to
    return --, with ``cross`` by a < first_new <= b -- ke_hamming_scan_cross.  ``calls`` records the tables it was given."""

    def __init__(self):
        self.calls = []

    def hamming_scan(self, hashes, n, *, ids=None, sizes=None, threshold=8, band_bits=16, band_count=4, size_ratio=0.0,
                     bucket_pair_cap=0, part_index=0, part_count=1, capacity=None, first_new=None, cross=False):
        self.calls.append(dict(n=int(n), first_new=first_new, cross=cross, hashes=np.array(hashes), ids=None if ids is None else np.array(ids),
                               sizes=None if sizes is None else np.array(sizes)))
        first_new = int(first_new or 0)
        if n < 2:
            return np.zeros(0, EDGE_DTYPE), np.zeros(4, np.uint64)
        edges, c = O.scan_banded(hashes, ids=None, sizes=sizes, threshold=threshold, band_bits=band_bits, band_count=band_count,
                                 size_ratio=size_ratio, bucket_pair_cap=bucket_pair_cap)
        if ids is not None:
            edges = edges[ids[edges["a"]] != ids[edges["b"]]]
        edges = edges[(edges["a"] < first_new) & (edges["b"] >= first_new)] if cross else edges[edges["b"] >= first_new]
        out = np.zeros(len(edges), EDGE_DTYPE)
        for k in ("a", "b", "h", "bands"):
            out[k] = edges[k]
        return out, np.array([0, 0, len(out), int(c[0])], np.uint64)
