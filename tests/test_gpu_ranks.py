"""The ``devices=`` keyword of the real-file seams on the GPU: N = 2 and 3 rank workers (kobato_eyes_amd/ranks.py) that share
device 0 -- the rehearsal a one-GPU box allows -- against the same call with ``devices=None``.  The worker processes are started
once per N for the whole module; the cases where a worker dies or falls silent are tests/test_ranks_cpu.py's, against stand-ins."""
from __future__ import annotations

import dataclasses
import os
import sqlite3

import numpy as np
import pytest

import _golden as G

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")

STAGES = ["Loading files", "Computing signatures", "Building groups", "Clustering duplicates"]
SIGNATURES = "CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER NOT NULL, dhash_u64 INTEGER NOT NULL)"


@pytest.fixture(scope="module")
def K():
    import kobato_eyes_amd

    kobato_eyes_amd._native.get_context(0)
    return kobato_eyes_amd


@pytest.fixture(scope="module")
def pools(K):
    """[0, 0] and [0, 0, 0]: where the seams' ``devices=`` finds them, every request under a 120 s limit."""
    from kobato_eyes_amd import ranks

    ranks.shutdown()
    yield {n: ranks.get_pool([0] * n, timeout=120) for n in (2, 3)}
    ranks.shutdown()


@pytest.fixture(scope="module")
def corpus(K, tmp_path_factory):
    """The 85 files of every route, their expected rows (the reference's), and this build's rows on one device."""
    tasks, expected = G.write_worker_corpus(tmp_path_factory.mktemp("worker_corpus"))
    patch = pytest.MonkeyPatch()
    patch.setenv("KE_FUSED_MIN_IMAGES", "1")                  # as tests/conftest.py sets it for every test
    try:
        single = K.compute_signatures_mp(tasks, max_workers=4, chunksize=16)
    finally:
        patch.undo()
    return tasks, expected, single


def _fresh_db(path) -> str:
    conn = sqlite3.connect(path)
    conn.execute(SIGNATURES)
    conn.commit()
    conn.close()
    return str(path)


def _stored(db):
    conn = sqlite3.connect(db)
    try:
        return conn.execute("SELECT file_id, phash_u64, dhash_u64 FROM signatures ORDER BY file_id").fetchall()
    finally:
        conn.close()


@pytest.mark.parametrize("n", [2, 3])
def test_worker_corpus_rows_equal_the_single_device_rows_and_the_reference(K, pools, corpus, n):
    from kobato_eyes_amd import fastsig

    tasks, expected, single = corpus
    seen = []
    rows = K.compute_signatures_mp(tasks, max_workers=4, chunksize=16, rank_chunk=16, devices=[0] * n,
                                   progress=lambda d, t: seen.append((d, t)))
    assert type(rows) is fastsig._SignedRows
    assert [r[0] for r in rows] == [r[0] for r in expected]                  # the same files dropped, input order kept
    by_name = {fid: os.path.basename(p) for fid, p in tasks}
    wrong = [by_name[a[0]] for a, b in zip(rows, expected) if tuple(a) != tuple(b)]
    assert not wrong, wrong
    assert rows == single
    assert len(tasks) == 85 and seen[-1] == (85, 85)
    assert not pools[n].closed


@pytest.mark.parametrize("n", [2, 3])
def test_an_environment_set_after_the_pool_started_reaches_the_workers(K, pools, corpus, monkeypatch, n):
    tasks, expected, single = corpus
    monkeypatch.setenv("KE_DECODE_PROCESS_MIN", "100000")
    monkeypatch.setenv("KE_GPU_JPEG", "0")                    # the Pillow route, as "pillow_threads" of tests/test_gpu_seams.py
    monkeypatch.setenv("KE_GPU_PNG", "0")
    rows = K.compute_signatures_mp(tasks, max_workers=4, chunksize=16, rank_chunk=16, devices=[0] * n)
    assert rows == single and [tuple(r) for r in rows] == [tuple(r) for r in expected]
    for reply in pools[n].ask_all({"op": "env"}):
        assert reply["env"].get("KE_GPU_JPEG") == "0" and reply["env"].get("KE_GPU_PNG") == "0"
        assert reply["pid"] != os.getpid()


@pytest.mark.parametrize("n", [2, 3])
def test_cancel_returns_a_strict_prefix(K, pools, corpus, n):
    tasks, expected, single = corpus
    asked = {"n": 0}

    def cancel():
        asked["n"] += 1
        return asked["n"] > 3

    out = K.compute_signatures_mp(tasks, max_workers=4, chunksize=16, rank_chunk=16, devices=[0] * n, cancel_fn=cancel)
    assert len(out) < len(single) and out == single[:len(out)]
    assert K.compute_signatures_mp(tasks, max_workers=4, chunksize=16, devices=[0] * n, cancel_fn=lambda: True) == []


def test_fast_fill_stores_the_rows_of_the_single_device_call(K, pools, corpus, tmp_path):
    tasks, expected, single = corpus
    one, two = _fresh_db(tmp_path / "one.db"), _fresh_db(tmp_path / "two.db")
    rows_one = K.fast_fill_missing_signatures(one, tasks, max_workers=4, chunksize=16)
    rows_two = K.fast_fill_missing_signatures(two, tasks, max_workers=4, chunksize=16, rank_chunk=16, devices=[0, 0])
    assert rows_two == rows_one == single
    assert _stored(two) == _stored(one) and len(_stored(two)) == len(expected)


def test_refine_pairs_equals_the_single_device_call_field_for_field(K, pools, tmp_path):
    from oracle import oracle as O

    rng = np.random.default_rng(3)
    base = O.synth_rgb(4242, 96, 80)
    files = []
    for k in range(8):
        px = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) if k % 2 else base
        p = tmp_path / (f"r{k}.jpg" if k in (0, 3, 4, 7) else f"r{k}.png")
        Image.fromarray(px).save(p, **({"quality": 92} if p.suffix == ".jpg" else {}))
        files.append(p)
    pairs = [(a, b, files[a], files[b]) for a, b in [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 5), (3, 7)]]
    th = K.RefinementThresholds(ssim=0.9)
    want_stats, stats = {}, {}
    want = K.refine_pairs(pairs, thresholds=th, stats=want_stats)
    got = K.refine_pairs(pairs, thresholds=th, stats=stats, devices=[0, 0])
    assert all(m is not None and m.ssim is not None for m in want)
    assert [dataclasses.asdict(m) for m in got] == [dataclasses.asdict(m) for m in want] and got == want
    assert [(m.file_id_a, m.file_id_b) for m in got] == [(a, b) for a, b, _, _ in pairs]
    assert stats["pairs"] == 7 == want_stats["pairs"]
    assert stats["decodes"] >= want_stats["decodes"] == 8     # a file that two blocks need is decoded by both workers
    assert stats["gpu_decodes"] >= want_stats["gpu_decodes"]


def test_run_duplicate_scan_equals_the_single_device_scan(K, pools, tmp_path):
    from oracle import oracle as O

    g = G.config0_golden()
    side, count = g["side"], 200
    batch = O.synth_rgb_batch(0, count, side, side)
    rows = []
    for k, r in enumerate(g["rows"][:count]):
        p = tmp_path / r["path"]
        Image.fromarray(batch[k]).save(p, compress_level=1)
        rows.append(dict(r, path=str(p), phash_u64=None))
    listings, stored = [], []
    for name, devices in (("one.db", None), ("two.db", [0, 0])):
        db = _fresh_db(tmp_path / name)
        stages = []
        clusters = K.run_duplicate_scan(rows, db_path=db, config=K.DuplicateScanConfig(hamming_threshold=8),
                                        progress=lambda s, d, t: stages.append(s), devices=devices)
        listings.append([{"keeper_id": c.keeper_id, "entries": [[e.file.file_id, e.best_hamming] for e in c.files]} for c in clusters])
        stored.append(_stored(db))
        assert [s for k, s in enumerate(stages) if k == 0 or stages[k - 1] != s] == STAGES
    assert listings[1] == listings[0]
    assert stored[1] == stored[0] and len(stored[1]) == count
    assert stored[1] == [(i + 1, p, d) for i, (p, d) in enumerate(zip(g["phash_s64"][:count], g["dhash_s64"][:count]))]
