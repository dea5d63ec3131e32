"""bench.py itself: the helpers behind `--dump-outputs` (CPU) and a plain run with `--dump-outputs` on a small corpus,
its outputs held against the CPU oracle (GPU)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402


def test_hash_words_are_exact():
    h = np.array([0, 1, 0xFFFFFFFF, 1 << 32, 0x8000000000000001, 0xFFFFFFFFFFFFFFFF], np.uint64)
    w = bench.hash_words(h.view(np.int64))
    assert w.dtype == np.float64 and w.shape == (len(h), 2)
    back = (w[:, 0].astype(np.uint64) << np.uint64(32)) | w[:, 1].astype(np.uint64)
    assert np.array_equal(back, h)


def test_edge_rows_are_sorted_and_keep_their_order():
    from kobato_eyes_amd import _native

    e = np.zeros(4, _native.EDGE_DTYPE)
    e["a"], e["b"], e["h"], e["bands"] = [5, 1, 5, 1], [9, 7, 6, 3], [1, 2, 3, 4], [1, 1, 2, 2]
    rows, order = bench.edge_rows(e)
    assert rows.dtype == np.float64
    assert rows.tolist() == [[1, 3, 4, 2], [1, 7, 2, 1], [5, 6, 3, 2], [5, 9, 1, 1]]
    assert order.tolist() == [3, 1, 2, 0]
    assert bench.edge_rows(np.zeros(0, _native.EDGE_DTYPE))[0].shape == (0, 4)


def test_dump_outputs_samples_the_same_rows_past_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8000)
    arrays = {"big": np.arange(2000, dtype=np.float64), "pairs": np.arange(4000, dtype=np.float64).reshape(2000, 2),
              "small": np.ones(3, np.float32)}
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "one" / f"{n}.npy") for n in arrays}
    assert sum(a.nbytes for a in got.values()) <= 8000
    assert got["big"].dtype == np.float64 and got["small"].dtype == np.float32
    assert np.array_equal(got["pairs"][:, 0] / 2, got["big"])              # same rows for arrays of the same length
    assert np.all(np.diff(got["big"]) > 0) and len(got["big"]) > 0
    for n in arrays:
        assert np.array_equal(got[n], np.load(tmp_path / "two" / f"{n}.npy"))
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 60_000_000)            # inside the budget: written whole
    bench.dump_outputs(str(tmp_path / "whole"), {"big": arrays["big"]})
    assert np.array_equal(np.load(tmp_path / "whole" / "big.npy"), arrays["big"])


@pytest.mark.gpu
def test_plain_run_times_the_step_and_dumps_what_it_computed(tmp_path):
    """A plain run prints the headline line without the --full extras; --dump-outputs writes the last timed step's hash
    table, edges and labels, equal to the oracle's on the same seeded corpus."""
    from oracle import oracle as O

    n, side, thr = 6000, 256, 8
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--images", str(n),
                          "--side", str(side), "--threshold", str(thr), "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True
    assert {"metric", "unit", "dtype"} <= set(out)
    assert not {"cpu_baseline", "phase_ms", "roofline_dual", "h2d_inclusive", "decode_inclusive", "phash_near_ties"} & set(out)

    d = tmp_path / "out"
    files = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(files) == {"phash", "edges", "labels", "scan_pairs", "margin"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000_000
    w = files["phash"]
    ph = (w[:, 0].astype(np.uint64) << np.uint64(32)) | w[:, 1].astype(np.uint64)
    k = 256                                                                 # the oracle's hashes of a prefix (host memory)
    exp_p, _ = O.hash_batch(O.synth_rgb_batch(0, k, side, side), want_dhash=False)
    assert ph.shape == (n,) and np.array_equal(ph[:k], np.asarray(exp_p, np.uint64))
    exp_e, _ = O.scan_banded(ph, threshold=thr)
    edges = files["edges"].astype(np.int64)
    assert len(edges) == out["edges"]
    assert edges[:, :3].tolist() == sorted(map(list, exp_e[["a", "b", "h"]].tolist()))
    labels = files["labels"].astype(np.int64)
    assert labels.shape == (n,) and np.all(labels <= np.arange(n))
    assert np.array_equal(labels[edges[:, 0]], labels[edges[:, 1]])
    assert files["margin"].shape == (n,)
