"""The rank-worker pool (kobato_eyes_amd/ranks.py) and the ``devices=`` keyword of the seams, without a GPU and without the
library: the workers are stand-ins (tests/_ranks_fake_worker.py), started through the same Popen path as the real ones."""
from __future__ import annotations

import json
import os
import sys
import time

import pytest

FAKE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ranks_fake_worker.py")


@pytest.fixture()
def R():
    from kobato_eyes_amd import ranks

    ranks.shutdown()
    yield ranks
    ranks.shutdown()


def _start(R, devices, tmp_path, script=None, timeout=30):
    """A pool of stand-ins in the cache, where the seams' ``devices=`` finds it."""
    return R.get_pool(devices, timeout=timeout, command=[sys.executable, FAKE, "--script", json.dumps(script or {}), "--log", str(tmp_path)])


def _log(tmp_path, rank):
    p = tmp_path / f"rank{rank}.log"
    return [json.loads(line) for line in p.read_text().splitlines()] if p.exists() else []


def _gone(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return True
    return False


def _tasks(total):
    return [(k, f"f{k}") for k in range(1, total + 1)]


def _rows(total):
    return [(k, 3 * k, -k) for k in range(1, total + 1) if k % 50]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_rows_come_back_in_input_order_whatever_order_the_chunks_arrive_in(R, tmp_path, n):
    import kobato_eyes_amd.fastsig as fs

    # worker 0 sits on its first and third chunk while the others run ahead: chunk 0 arrives after chunks 1, 2, 3 ...
    _start(R, [0] * n, tmp_path, {"delays": {"0": [0.2, 0, 0.1], "1": [0, 0.05]}})
    rows = fs.compute_signatures_mp(_tasks(1000), max_workers=8, chunksize=16, rank_chunk=64, devices=[0] * n)
    assert type(rows) is fs._SignedRows
    assert rows == _rows(1000)
    logs = [_log(tmp_path, k) for k in range(n)]
    assert sum(len(entries) for entries in logs) == 16 and all(entries for entries in logs)      # 16 chunks, dealt on demand
    assert {e["workers"] for entries in logs for e in entries} == {max(1, 8 // n)}               # the caller's CPUs, divided


def test_default_rank_chunk_gives_every_worker_one_chunk(R, tmp_path):
    import kobato_eyes_amd.fastsig as fs

    _start(R, [0, 0, 0], tmp_path)
    assert fs.compute_signatures_mp(_tasks(100), max_workers=2, devices=[0, 0, 0]) == _rows(100)
    assert [len(_log(tmp_path, k)) for k in range(3)] == [1, 1, 1]           # ceil(100 / 3) = 34, 34, 32
    assert {e["workers"] for k in range(3) for e in _log(tmp_path, k)} == {1}


@pytest.mark.parametrize("n", [1, 3])
def test_progress_marks_are_those_of_the_single_device_path(R, tmp_path, n):
    import kobato_eyes_amd.fastsig as fs

    _start(R, [0] * n, tmp_path, {"delays": {"0": [0.05]}})
    for total, marks in ((450, [200, 400, 450]), (400, [200, 400]), (199, [199]), (128, [128])):
        seen = []
        rows = fs.compute_signatures_mp(_tasks(total), rank_chunk=64, devices=[0] * n, progress=lambda d, t: seen.append((d, t)))
        assert seen == [(m, total) for m in marks]
        assert rows == _rows(total)


@pytest.mark.parametrize("n", [1, 3])
def test_cancel_returns_the_prefix_of_whole_chunks(R, tmp_path, n):
    import kobato_eyes_amd.fastsig as fs

    # worker 0 answers at once, the others late: chunk 0 is whole by the third message
    _start(R, [0] * n, tmp_path, {"delays": {"1": [0.6, 0.6], "2": [0.6, 0.6]}})
    full = _rows(1000)
    asked = {"n": 0}

    def cancel():
        asked["n"] += 1
        return asked["n"] > 4                                  # once before anything is sent, then after each message: true after the 3rd

    out = fs.compute_signatures_mp(_tasks(1000), rank_chunk=64, devices=[0] * n, cancel_fn=cancel)
    assert 0 < len(out) < len(full) and out == full[:len(out)]
    assert type(out) is fs._SignedRows
    assert all(e["stream"] for k in range(n) for e in _log(tmp_path, k))
    dealt = sum(len(_log(tmp_path, k)) for k in range(n))
    assert dealt < 16                                          # no new chunk after the answer was true
    # the pool is at rest and usable
    assert fs.compute_signatures_mp(_tasks(130), rank_chunk=64, devices=[0] * n) == _rows(130)


def test_cancel_from_the_start_sends_no_request(R, tmp_path):
    import kobato_eyes_amd.fastsig as fs

    _start(R, [0, 0], tmp_path)
    assert fs.compute_signatures_mp(_tasks(1000), rank_chunk=64, devices=[0, 0], cancel_fn=lambda: True) == []
    assert _log(tmp_path, 0) == [] and _log(tmp_path, 1) == []
    assert fs.compute_signatures_mp([], devices=[0, 0]) == []
    assert _log(tmp_path, 0) == [] and _log(tmp_path, 1) == []


def test_every_request_carries_the_callers_ke_environment(R, tmp_path, monkeypatch):
    monkeypatch.setenv("KE_RANKS_BEFORE", "1")
    pool = _start(R, [0, 1], tmp_path)
    first = pool.ask_all({"op": "env"})
    assert [r["device"] for r in first] == [0, 1]
    assert all(r["env"].get("KE_RANKS_BEFORE") == "1" and "KE_RANKS_AFTER" not in r["env"] for r in first)
    monkeypatch.setenv("KE_RANKS_AFTER", "set later")          # after the pool started
    monkeypatch.delenv("KE_RANKS_BEFORE")
    monkeypatch.setenv("RANKS_TEST_OTHER", "not ours")
    for r in pool.ask_all({"op": "env"}):
        assert r["env"].get("KE_RANKS_AFTER") == "set later"
        assert "KE_RANKS_BEFORE" not in r["env"]
        assert r["other"] is None
        assert r["env"] == {k: v for k, v in os.environ.items() if k.startswith("KE_")}


def test_a_worker_that_exits_ends_the_call_and_the_pool(R, tmp_path):
    import kobato_eyes_amd.fastsig as fs

    devices = [0, 1, 2]
    pool = _start(R, devices, tmp_path, {"exit": {"rank": 1, "request": 1, "status": 3}, "delays": {"0": [0, 5], "2": [0, 5]}})
    pids = [w.pid for w in pool.workers]
    with pytest.raises(RuntimeError) as failure:
        fs.compute_signatures_mp(_tasks(1000), rank_chunk=64, devices=devices)
    assert "exit status 3" in str(failure.value) and "device 1" in str(failure.value)
    assert all(_gone(pid) for pid in pids)
    assert R.cached_pool(devices) is None and pool.closed
    assert sum(len(_log(tmp_path, k)) for k in range(3)) < 16                # the rest of the work was not dealt to anybody


def test_a_silent_worker_ends_the_call_after_the_timeout(R, tmp_path):
    import kobato_eyes_amd.fastsig as fs

    devices = [0, 1]
    pool = _start(R, devices, tmp_path, {"sleep": {"rank": 1, "request": 0, "seconds": 60}}, timeout=2)
    pids = [w.pid for w in pool.workers]
    t0 = time.monotonic()
    with pytest.raises(RuntimeError) as failure:
        fs.compute_signatures_mp(_tasks(200), rank_chunk=64, devices=devices)
    took = time.monotonic() - t0
    assert 2 <= took < 2 + R.KILL_WAIT * len(devices) + 2, took
    assert "device 1" in str(failure.value) and "2 s" in str(failure.value)
    assert all(_gone(pid) for pid in pids)
    assert R.cached_pool(devices) is None


def test_an_exception_in_a_worker_is_raised_in_the_caller_and_the_pool_stays(R, tmp_path):
    import kobato_eyes_amd.fastsig as fs

    devices = [0, 0]
    pool = _start(R, devices, tmp_path, {"raise": {"rank": 1, "request": 0}})
    with pytest.raises(ValueError, match="^x$"):
        fs.compute_signatures_mp(_tasks(1000), rank_chunk=64, devices=devices)
    assert R.cached_pool(devices) is pool and not pool.closed
    assert fs.compute_signatures_mp(_tasks(300), rank_chunk=64, devices=devices) == _rows(300)


def test_limits_on_devices_and_shutdown(R, tmp_path, monkeypatch):
    import kobato_eyes_amd as K
    import kobato_eyes_amd.fastsig as fs

    started = []
    monkeypatch.setattr(R.subprocess, "Popen", lambda *a, **k: started.append(a) or (_ for _ in ()).throw(AssertionError("started")))
    for call in (lambda d: fs.compute_signatures_mp(_tasks(10), devices=d),
                 lambda d: fs.fast_fill_missing_signatures(str(tmp_path / "x.db"), _tasks(10), devices=d),
                 lambda d: K.refine_pairs([(1, 2, "a", "b")], devices=d),
                 lambda d: R.get_pool(d)):
        with pytest.raises(ValueError):
            call([0] * 16)
        with pytest.raises(ValueError):
            call([])
    assert not started
    monkeypatch.undo()
    pool = _start(R, [0] * 15, tmp_path)                       # fifteen is allowed
    pids = [w.pid for w in pool.workers]
    assert len(pids) == 15 and not any(_gone(pid) for pid in pids)
    t0 = time.monotonic()
    R.shutdown()
    assert time.monotonic() - t0 < R.QUIT_WAIT                 # they left on the quit message, nobody had to be terminated
    assert all(_gone(pid) for pid in pids)
    assert R.cached_pool([0] * 15) is None
    with pytest.raises(RuntimeError):
        pool.ask_all({"op": "env"})


def test_pairs_are_cut_into_contiguous_blocks_of_about_equal_size(R):
    sizes = {"a": 100, "b": 100, "c": 10, "d": 10, "e": 10, "f": 10, "g": 300, "h": 10, "i": 10, "j": 10, "k": 10}
    names = list(sizes)
    pairs = [(k, k + 1, names[k], names[k + 1]) for k in range(10)]        # neighbours share a file
    for n in range(1, 16):
        blocks = R.split_pairs(pairs, n, size_of=sizes.__getitem__)
        assert len(blocks) == min(n, 10)
        assert blocks[0][0] == 0 and blocks[-1][1] == 10
        assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))       # contiguous, every pair once
        assert all(lo < hi for lo, hi in blocks)                           # never empty
    # a pair weighs what it adds: 200, 10, 10, 10, 10, 300, 10, 10, 10, 10 -- two blocks of 240 and 340, not 5 + 5 by chance
    assert R.split_pairs(pairs, 2, size_of=sizes.__getitem__) == [(0, 5), (5, 10)]
    assert R.split_pairs(pairs, 3, size_of=sizes.__getitem__) == [(0, 1), (1, 5), (5, 10)]
    assert R.split_pairs(pairs, 4, size_of=lambda p: 0) == [(0, 2), (2, 5), (5, 7), (7, 10)]   # nothing known: by count
    assert R.split_pairs([], 3, size_of=sizes.__getitem__) == []


def test_refined_blocks_are_joined_in_input_order_and_their_stats_summed(R, tmp_path):
    import kobato_eyes_amd as K

    files = []
    for k in range(11):
        p = tmp_path / f"f{k}.bin"
        p.write_bytes(b"\0" * (1000 if k == 6 else 100))
        files.append(str(p))
    pairs = [(k, k + 1, files[k], files[k + 1]) for k in range(10)]
    _start(R, [0, 1, 2], tmp_path)
    stats = {}
    out = K.refine_pairs(pairs, io_workers=7, stats=stats, devices=[0, 1, 2])
    assert [(m[1], m[2]) for m in out] == [(k, k + 1) for k in range(10)]
    ranks_of = [m[3] for m in out]
    assert ranks_of == sorted(ranks_of) and set(ranks_of) == {0, 1, 2}     # one contiguous block per worker
    assert stats["pairs"] == 10 and stats["fit_launches"] == 3 and stats["ssim_launches"] == 3
    assert stats["decodes"] == 11 + 2                                      # a file on a block's edge counts once per worker
    assert {e["io_workers"] for k in range(3) for e in _log(tmp_path, k)} == {2}
    stats = {}
    assert K.refine_pairs([], stats=stats, devices=[0, 1, 2]) == [] and stats["pairs"] == 0
    assert [m[3] for m in K.refine_pairs(pairs[:2], devices=[0, 1, 2])] == [0, 1]       # fewer pairs than workers


def test_scan_dups_takes_a_devices_list(monkeypatch, capsys):
    from kobato_eyes_amd import cli

    seen = {}
    monkeypatch.setattr(cli, "scan_database", lambda db, **kw: seen.update(kw, db=db) or [])
    assert cli.main(["scan-dups", "--db", "k.db", "--devices", "0,1,2"]) == 0
    assert seen["devices"] == [0, 1, 2] and seen["device"] is None            # the scan then runs on devices[0]
    assert cli.main(["scan-dups", "--db", "k.db", "--device", "1"]) == 0
    assert seen["devices"] is None and seen["device"] == 1
