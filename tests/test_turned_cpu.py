"""Turned pHashes and the cross scan without a GPU.

* The precondition of tests/test_gpu_turned.py, on the CPU oracle alone: for every image that file uses, the pHash made
  from orientation k of the image's 32x32 tile lies at most 2 bits from the pHash of the really turned image for every k
  and 0 bits for the three flips (the bound is the largest value seen on the 24 images of the issue's measurement), and the
  image's own pHash lies more than 8 bits from each of its seven turned hashes -- no symmetric picture among the inputs.
* turn_k by the issue's definition against Pillow's Image.transpose under the names table.
* csrc/ke_scan_region.h's cross region in a stand-alone host program (tests/_scan_cross_cpu.cpp), plain and with
  AddressSanitizer + UBSan.
* DuplicateScanner.turned_edges and api.find_turned_duplicates against a stand-in context whose hamming_scan is the
  oracle's banded scan filtered by a < first_new <= b -- what ke_hamming_scan_cross is specified to return."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _scan_from_cases as S
import _turned_cases as T
from _scan_standin import OracleScanContext
from kobato_eyes_amd import _native, api, cli, turned
from kobato_eyes_amd.scanner import DuplicateFile, DuplicateScanConfig, DuplicateScanner, TurnedMatch
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
MASK = (1 << 64) - 1


# ---- definitions ------------------------------------------------------------------------------------------------------
def test_turn_k_is_pillows_transpose_under_the_names_table():
    from PIL import Image

    a = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    im = Image.fromarray(a)
    assert turned.ORIENTATIONS[0][1] is None and len(turned.ORIENTATIONS) == 8
    for k in range(1, 8):
        want = np.asarray(im.transpose(getattr(Image.Transpose, turned.ORIENTATIONS[k][1])))
        assert np.array_equal(T.turn_k(k, a), want), turned.ORIENTATIONS[k]
        assert np.array_equal(turned.turn(k, a), want), turned.ORIENTATIONS[k]
    assert [turned.ORIENTATIONS[k][1] for k in (5, 6)] == ["ROTATE_270", "ROTATE_90"]      # clockwise, counter-clockwise


def test_inverse_and_compose():
    a = np.arange(6).reshape(2, 3)
    assert turned.INVERSE == (0, 1, 2, 3, 4, 6, 5, 7)
    for k in range(8):
        assert np.array_equal(T.turn_k(turned.INVERSE[k], T.turn_k(k, a)), a)
        for j in range(8):
            assert np.array_equal(T.turn_k(turned.COMPOSE[j][k], a), T.turn_k(k, T.turn_k(j, a)))


# ---- the precondition of the GPU tests ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hash_images", "file_pictures"])
def test_tile_hashes_stand_for_the_turned_images_hashes(which):
    worst = 0
    for i, px in enumerate(getattr(T, which)()):
        own, _, tile, _, _ = O.hash_image(px, want_tiles=True)
        for k in range(8):
            from_tile = O.phash_from_tile(T.turn_k(k, tile))[0]
            real = O.hash_image(T.turn_k(k, px))[0]
            d = O.hamming64(from_tile, real)
            worst = max(worst, d)
            assert d <= (0 if k < 4 else 2), (which, i, px.shape, k, d)
            if k == 0:
                assert from_tile == own
            else:
                assert O.hamming64(own, from_tile) > T.THRESHOLD, (which, i, px.shape, k)
    print(f"{which}: largest distance between a tile's turned hash and the turned image's hash = {worst}")


# ---- the cross region ---------------------------------------------------------------------------------------------------
def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_the_cross_region_arithmetic_holds(tmp_path, flags):
    exe = str(tmp_path / "scan_cross_cpu")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-O1", "-g", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "_scan_cross_cpu.cpp"), "-o", exe])
    res = subprocess.run([exe, *map(str, S.FIRST_NEW)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    cases = sum(1 for n in (1, 2, 1023, 1024, 1025, 2500, 5000) for f in (*S.FIRST_NEW, n - 1) if 0 <= f <= n)
    assert res.stdout.strip().splitlines()[-1] == f"ok cases={cases}", res.stdout[-2000:]


# ---- turned_edges and find_turned_duplicates against the oracle's scan ------------------------------------------------------
class _Context(OracleScanContext):
    """The shared stand-in, with ``calls`` as the (n, first_new, cross) these tests compare."""

    def hamming_scan(self, hashes, n, **keywords):
        out = super().hamming_scan(hashes, n, **keywords)
        self.calls[-1] = (int(n), keywords.get("first_new"), keywords.get("cross", False))
        return out


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.delenv("KE_DUP_BUCKET_PAIR_CAP", raising=False)
    c = _Context()
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": c)
    return c


def _file(fid, phash, size=1000):
    return DuplicateFile(fid, Path(f"lib/f{fid:04d}.png"), size, 100, 100, int(phash) & MASK)


def _bits(*positions):
    v = 0
    for p in positions:
        v |= 1 << p
    return v


def _table(rng, n):
    """n files with random stored hashes and random turned rows (column 0 = the stored hash): nothing matches by chance."""
    t = rng.integers(0, 1 << 64, size=(n, 8), dtype=np.uint64)
    files = [_file(10 + i, int(t[i, 0])) for i in range(n)]
    return files, t


def _scanner():
    return DuplicateScanner(DuplicateScanConfig(hamming_threshold=T.THRESHOLD))


def test_positions_map_to_file_and_orientation(ctx):
    """Entry n + 7 * s + (k - 1) of the table is orientation k of file s: planted one at a time for every (s, k)."""
    rng = np.random.default_rng(1)
    for s in (0, 3, 5):
        for k in range(1, 8):
            files, t = _table(rng, 6)
            a = 1 if s != 1 else 2
            t[s, k] = np.uint64((files[a].phash ^ _bits(20, 40, 63)) & MASK)          # file a looks like orientation k of file s
            got = _scanner().turned_edges(files, t)
            lo, hi = sorted((files[a].file_id, files[s].file_id))
            want_k = k if files[a].file_id < files[s].file_id else turned.INVERSE[k]
            assert got == [TurnedMatch(lo, hi, want_k, 3)], (s, k, got)
            assert ctx.calls[-1] == (6 + 42, 6, True)


def test_a_match_found_from_the_larger_id_goes_through_inverse(ctx):
    rng = np.random.default_rng(2)
    files, t = _table(rng, 4)
    t[0, 5] = np.uint64(files[3].phash)                  # file 13 is the clockwise quarter turn of file 10's picture ...
    got = _scanner().turned_edges(files, t)
    assert got == [TurnedMatch(10, 13, 6, 0)]            # ... so turning 13's counter-clockwise gives 10's
    files, t = _table(rng, 4)
    t[3, 5] = np.uint64(files[0].phash)                  # file 10 is the clockwise quarter turn of file 13's picture
    assert _scanner().turned_edges(files, t) == [TurnedMatch(10, 13, 5, 0)]


def test_one_match_per_pair_smallest_hamming_then_smallest_orientation(ctx):
    rng = np.random.default_rng(3)
    files, t = _table(rng, 5)
    t[2, 3] = np.uint64((files[0].phash ^ _bits(30, 31)) & MASK)       # 2 bits through orientation 3
    t[2, 6] = np.uint64((files[0].phash ^ _bits(32)) & MASK)           # 1 bit through orientation 6: wins
    t[0, 1] = np.uint64((files[2].phash ^ _bits(33, 34, 35)) & MASK)   # the other way round, 3 bits
    t[4, 7] = np.uint64((files[1].phash ^ _bits(50)) & MASK)           # a tie on the distance: 7 from 14's side ...
    t[1, 2] = np.uint64((files[4].phash ^ _bits(51)) & MASK)           # ... and 2 from 11's side: the smaller orientation
    got = _scanner().turned_edges(files, t)
    assert got == [TurnedMatch(10, 12, 6, 1), TurnedMatch(11, 14, 2, 1)]


def test_a_file_without_turned_hashes_takes_part_with_its_stored_hash_only(ctx):
    rng = np.random.default_rng(4)
    files, t = _table(rng, 5)
    ok = np.array([True, False, True, True, True])
    t[1] = 0                                             # what turned_signatures leaves for a file Pillow cannot open
    t[1, 4] = np.uint64(files[3].phash)                  # must not be read
    t[4, 2] = np.uint64(files[1].phash)                  # file 11's stored hash still matches others' turned hashes
    t[3, 1] = np.uint64(files[0].phash)                  # a file behind the gap keeps its own row
    got = _scanner().turned_edges(files, t, ok)
    assert got == [TurnedMatch(10, 13, 1, 0), TurnedMatch(11, 14, 2, 0)]
    assert ctx.calls[-1] == (5 + 28, 5, True)
    assert _scanner().turned_edges(files, t, np.zeros(5, bool)) == []


def test_equal_ids_are_dropped(ctx):
    """A symmetric picture matches its own turned hash, and one file listed twice matches itself: the scan's id rule drops both."""
    rng = np.random.default_rng(5)
    files, t = _table(rng, 4)
    t[2, 1] = t[2, 0]                                    # left-right symmetric
    files[3] = DuplicateFile(files[1].file_id, files[1].path, 1000, 100, 100, files[1].phash)
    t[3, 2] = np.uint64(files[1].phash)
    assert _scanner().turned_edges(files, t) == []


def test_size_ratio_applies_to_a_turned_entry_through_its_source_file(ctx):
    rng = np.random.default_rng(6)
    files, t = _table(rng, 3)
    files[2] = _file(12, files[2].phash, size=100)
    t[2, 1] = np.uint64(files[0].phash)
    assert DuplicateScanner(DuplicateScanConfig(hamming_threshold=8, size_ratio=0.5)).turned_edges(files, t) == []
    assert DuplicateScanner(DuplicateScanConfig(hamming_threshold=8, size_ratio=0.05)).turned_edges(files, t) == [TurnedMatch(10, 12, 1, 0)]


def test_find_turned_duplicates_joins_plain_edges_and_matches(ctx, monkeypatch):
    rng = np.random.default_rng(7)
    files, t = _table(rng, 7)
    files[1] = _file(11, files[0].phash ^ _bits(20))     # a plain near-duplicate of file 10
    t[1, 0] = np.uint64(files[1].phash)
    t[4, 1] = np.uint64(files[0].phash ^ _bits(21, 22))  # file 14 mirrored looks like file 10
    t[6, 5] = np.uint64(files[5].phash)                  # file 15 is the clockwise turn of file 16's picture
    ok = np.ones(7, bool)
    ok[3] = False
    seen = {}

    def fake_signatures(paths, *, device=0):
        seen["paths"] = [str(p) for p in paths]
        return t, ok

    monkeypatch.setattr(turned, "turned_signatures", fake_signatures)
    clusters, matches = api.find_turned_duplicates(files, hamming_threshold=T.THRESHOLD)
    assert seen["paths"] == [str(f.path) for f in files]
    # file 11, one bit from file 10, lies three bits from file 14's mirrored hash
    assert matches == [TurnedMatch(10, 14, 1, 2), TurnedMatch(11, 14, 1, 3), TurnedMatch(15, 16, 5, 0)]
    groups = sorted(sorted(e.file.file_id for e in c.files) for c in clusters)
    assert groups == [[10, 11, 14], [15, 16]]
    best = {e.file.file_id: e.best_hamming for c in clusters for e in c.files}
    assert best == {10: 1, 11: 1, 14: 2, 15: 0, 16: 0}
    plain = api.find_duplicates(files, hamming_threshold=T.THRESHOLD)
    assert sorted(sorted(e.file.file_id for e in c.files) for c in plain) == [[10, 11]]
    # the CSV column: the turn that brings a file's picture to its group's keeper's
    by_id = {c.keeper_id: c for c in clusters}
    orient = cli.orientations_to_keeper(clusters, matches, {(10, 11)})
    for c in clusters:
        members = {e.file.file_id for e in c.files}
        if members == {15, 16}:
            assert orient.get(15 if c.keeper_id == 16 else 16) == (6 if c.keeper_id == 16 else 5)
        else:
            want = {10: {14: 1}, 11: {14: 1}, 14: {10: 1, 11: 1}}[c.keeper_id]
            assert {f: k for f, k in orient.items() if f in members} == want
    assert by_id


def test_cross_needs_first_new():
    with pytest.raises(ValueError):
        _native.Context.hamming_scan(object(), np.zeros(4, np.uint64), 4, cross=True)
