"""The arithmetic of ke_hamming_nearest without a GPU: csrc/ke_nearest_core.h compiled with the host C++ compiler
(tests/_nearest_core_cpu.cpp) into a temporary directory.

* The cut -- from a histogram of S by distance, k and max_distance: the distance d* the k-th entry lies at, how many entries
  are taken at d*, and the count -- against its restatement here, on every histogram over 3 bins with entries 0..3, every k in
  1..12 and every max_distance, and on 2 000 random 65-bin histograms: empty ones, everything in one bin, totals below k.
* The sort key packs and unpacks at positions 0 and 2^31 - 1 and distances 0 and 64, and ascending keys are (distance, position).
* The two-pass walk, driven on the host the way the kernel runs it, equals the definition (xor, popcount, lexsort, id filter).
* The same source has a ``main`` that holds the walk against the definition spelled out in C++ at table sizes 1, 255, 256, 257
  and 1 025; it is built with AddressSanitizer and UBSan and run as a program of its own, every buffer ending where its data
  ends.  Every comparison is exact equality of integers."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "_nearest_core_cpu.cpp")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nearest_core_cpu") / "nearest_core_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC, SOURCE, "-o", out])
    lib = C.CDLL(out)
    lib.nr_cut.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.nr_cut.restype = None
    lib.nr_within.argtypes = [C.c_void_p, C.c_int32]
    lib.nr_within.restype = C.c_int64
    lib.nr_key.argtypes = [C.c_uint32, C.c_uint32]
    lib.nr_key.restype = C.c_uint64
    lib.nr_key_distance.argtypes = [C.c_uint64]
    lib.nr_key_distance.restype = C.c_uint32
    lib.nr_key_position.argtypes = [C.c_uint64]
    lib.nr_key_position.restype = C.c_uint32
    lib.nr_seg_lo.argtypes = lib.nr_seg_hi.argtypes = [C.c_int64, C.c_int32]
    lib.nr_seg_lo.restype = lib.nr_seg_hi.restype = C.c_int64
    lib.nr_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nr_walk.restype = C.c_int64
    return lib


def cut_restated(hist, k: int, max_distance: int) -> tuple:
    """(d*, taken at d*, count): the entries within max_distance in order of distance, cut after the k-th."""
    upto = np.cumsum(np.asarray(hist, np.int64)[:max_distance + 1])     # entries at distance <= d
    if int(upto[-1]) < k:
        return max_distance + 1, 0, int(upto[-1])
    dstar = int(np.searchsorted(upto, k, side="left"))                  # the first distance with k entries at or below it
    return dstar, k - (int(upto[dstar - 1]) if dstar else 0), k


def cut_of(cpu, hist, k: int, max_distance: int) -> tuple:
    full = np.zeros(65, np.uint32)
    full[:len(hist)] = hist
    out = np.full(3, -7, np.int32)
    cpu.nr_cut(full.ctypes.data, k, max_distance, out.ctypes.data)
    return tuple(int(v) for v in out)


def test_the_limits_are_the_headers(cpu):
    header = open(os.path.join(ROOT, "include", "keyes.h")).read()
    assert f"#define KE_NEAREST_MAX_K {cpu.nr_max_k()}\n" in header and cpu.nr_max_k() == 1024
    assert cpu.nr_threads() == 256


def test_the_cut_on_every_small_histogram(cpu):
    cases = 0
    for hist in itertools.product(range(4), repeat=3):
        for k in range(1, 13):
            for max_distance in range(0, 65):
                got, want = cut_of(cpu, hist, k, max_distance), cut_restated(hist, k, max_distance)
                assert got == want, (hist, k, max_distance)
                assert got[2] == min(k, sum(hist[:max_distance + 1]))
                cases += 1
    assert cases == 64 * 12 * 65


def test_the_cut_on_random_histograms(cpu):
    rng = np.random.default_rng(20)
    kinds = {"empty": 0, "one_bin": 0, "below_k": 0, "cut_inside": 0}
    for case in range(2000):
        kind = case % 5
        hist = np.zeros(65, np.uint32)
        if kind == 1:
            hist[rng.integers(0, 65)] = rng.integers(1, 3000)
        elif kind == 2:
            hist[rng.integers(0, 65, 6)] = rng.integers(0, 3, 6)                      # a few entries: totals below most k
        elif kind >= 3:
            hist[:] = rng.integers(0, rng.choice([2, 40, 100000]), 65)
        k = int(rng.choice([1, 2, 7, 10, 64, 1000, 1024]))
        max_distance = int(rng.choice([0, 5, 12, 31, 63, 64]))
        got, want = cut_of(cpu, hist, k, max_distance), cut_restated(hist, k, max_distance)
        assert got == want, (case, k, max_distance)
        assert cpu.nr_within(hist.ctypes.data, max_distance) == int(hist[:max_distance + 1].sum())
        total = int(hist[:max_distance + 1].sum())
        kinds["empty"] += total == 0
        kinds["one_bin"] += kind == 1
        kinds["below_k"] += 0 < total < k
        kinds["cut_inside"] += total >= k and got[1] < int(hist[got[0]])
    assert all(v > 20 for v in kinds.values()), kinds


def test_the_key_round_trips_and_orders(cpu):
    for d in (0, 1, 64):
        for p in (0, 1, 2**31 - 1):
            key = cpu.nr_key(d, p)
            assert key == (d << 32 | p)
            assert (cpu.nr_key_distance(key), cpu.nr_key_position(key)) == (d, p)
    assert cpu.nr_key(0, 2**31 - 1) < cpu.nr_key(1, 0) < cpu.nr_key(1, 1) < cpu.nr_key(64, 0) < 2**64 - 1


def test_the_segments_tile_the_table(cpu):
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 10**6, 2**31 - 1):
        at = 0
        for wave in range(4):
            lo, hi = cpu.nr_seg_lo(n, wave), cpu.nr_seg_hi(n, wave)
            assert lo == at and lo <= hi <= n, (n, wave)
            assert lo % 64 == 0 or lo == n, (n, wave)
            at = hi
        assert at == n


def definition(hashes, query, k, max_distance, ids=None, qid=None):
    d = np.array([bin(int(h) ^ int(query)).count("1") for h in hashes], np.int64)
    keep = d <= max_distance
    if ids is not None and qid is not None:
        keep &= ids != qid
    pos = np.nonzero(keep)[0]
    order = np.lexsort((pos, d[pos]))
    pos = pos[order]
    hist = np.bincount(d[pos], minlength=65).astype(np.uint32)
    return pos[:k], d[pos][:k], len(pos), hist


def test_the_walk_is_the_definition(cpu):
    rng = np.random.default_rng(21)
    cases = 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 8200, 12300):     # the last three have whole blocks
        query = int(rng.integers(0, 2**64, dtype=np.uint64))
        hashes = rng.integers(0, 2**64, n, dtype=np.uint64)
        near = rng.integers(0, n, min(n, 200))
        for i in near:                                                              # planted 0..12 bits from the query
            flips = rng.choice(64, int(rng.integers(0, 13)), replace=False)
            hashes[i] = np.uint64(query ^ sum(1 << int(b) for b in flips))
        ids = rng.integers(0, max(1, n // 2), n).astype(np.int64)
        for k in (1, 2, 7, 64, 1024):
            for max_distance in (0, 5, 31, 64):
                for with_ids in (False, True):
                    qid = int(ids[int(near[0])])
                    index = np.full(k, -7, np.int64)
                    distance = np.full(k, -7, np.int32)
                    count = np.full(1, -7, np.int32)
                    within = np.full(1, -7, np.int64)
                    hist = np.full(65, 7, np.uint32)
                    faults = cpu.nr_walk(hashes.ctypes.data, ids.ctypes.data if with_ids else None, n, query, int(with_ids), qid, k,
                                         max_distance, index.ctypes.data, distance.ctypes.data, count.ctypes.data, within.ctypes.data,
                                         hist.ctypes.data)
                    assert faults == 0, (n, k, max_distance, with_ids)
                    pos, dist, total, want_hist = definition(hashes, query, k, max_distance, ids if with_ids else None, qid)
                    c = min(k, total)
                    assert int(count[0]) == c and int(within[0]) == total, (n, k, max_distance, with_ids)
                    assert np.array_equal(index[:c], pos) and np.array_equal(distance[:c], dist), (n, k, max_distance, with_ids)
                    assert np.all(index[c:] == -1) and np.all(distance[c:] == -1)
                    assert np.array_equal(hist, want_hist)
                    cases += 1
    assert cases == 13 * 5 * 4 * 2


def test_sanitised_program(tmp_path):
    exe = str(tmp_path / "nearest_core_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-DNEAREST_CORE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", CSRC, SOURCE, "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == f"ok {5 * 3 * 5 * 4 * 2}" and "runtime error" not in done.stderr
