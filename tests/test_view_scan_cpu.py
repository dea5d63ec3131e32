"""DuplicateScanner's one view scan against a brute-force restatement of the three docstrings, without a GPU.

turned_edges, trimmed_edges and turned_trimmed_edges run against the stand-in context whose hamming_scan is the host oracle's
(_scan_standin.py), part_count = 1.  What they must return is written down here a second time, from the docstrings alone and
without table positions: every ordered pair of distinct files (x, y), every view of x as it lies against every view of y the mode
allows, kept where the hamming distance is within the threshold, one of the four 16-bit bands is equal, the ids differ and the
size ratio passes; the smaller id first, flags exchanged and the orientation through INVERSE; the smallest (hamming, orientation,
trimmed_a, trimmed_b) per pair.

The 14 files have shuffled ids.  Every hash is a filler word -- drawn once from a seeded generator, some 32 bits from every other
-- unless planted below: a copy of another file's stored hash with a few named bits flipped.  The brute force is asked for each
planted case by name, so the comparison cannot pass on an empty table."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from _scan_standin import OracleScanContext
from kobato_eyes_amd import _native
from kobato_eyes_amd.scanner import DuplicateFile, DuplicateScanConfig, DuplicateScanner, TransformedMatch, TrimmedMatch, TurnedMatch

THRESHOLD = 8
MASK = (1 << 64) - 1
INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)                    # the two quarter turns undo each other (turned.py's docstring)
IDS = [907, 12, 455, 33, 810, 78, 301, 64, 590, 5, 222, 149, 700, 410]
N = len(IDS)


def _flip(word, *bits):
    for b in bits:
        word = int(word) ^ (1 << b)
    return np.uint64(word & MASK)


def _inputs():
    rng = np.random.default_rng(2201)
    stored = rng.integers(0, 1 << 64, N, dtype=np.uint64)
    turned = rng.integers(0, 1 << 64, (N, 8), dtype=np.uint64)
    cut = rng.integers(0, 1 << 64, (N, 8), dtype=np.uint64)
    turned[:, 0] = stored
    ok, has = np.ones(N, bool), np.ones(N, bool)
    sizes = [1000] * N
    # found only from the larger id's side: 907 as it lies is the clockwise quarter turn of 12 (k = 5), 455 the counter-clockwise
    # one of 33 (k = 6) -- whole, and 455 also of the crop of 33
    turned[1, 5] = _flip(stored[0], 3, 40)
    turned[3, 6] = _flip(stored[2], 21)
    cut[3, 6] = _flip(stored[2], 21, 22, 60)
    # 78 / 810: one bit apart through orientation 2 from one side and through orientation 3 from the other
    turned[5, 3] = _flip(stored[4], 7)
    turned[4, 2] = _flip(stored[5], 50)
    # 64 / 301: each one's crop is one bit from the other as it lies, at orientation 0 and at the transpose
    cut[6, 0], cut[7, 0] = _flip(stored[7], 11), _flip(stored[6], 44)
    cut[6, 4], cut[7, 4] = _flip(stored[7], 12), _flip(stored[6], 45)
    # 590 has no turned hashes and 5 no qualifying box: what their rows hold must not be read, their stored hashes still take part
    ok[8], has[9] = False, False
    turned[8, 2] = stored[9]
    cut[9, 0], cut[9, 3] = stored[8], stored[8]
    turned[10, 1] = _flip(stored[8], 9)
    cut[10, 7] = _flip(stored[9], 30, 31)
    # 149 is symmetric left to right and trimmed by a hair: its mirrored hash and its crop's hash are its own
    turned[11, 1], cut[11, 0], cut[11, 1] = stored[11], stored[11], stored[11]
    # 700 / 410: a third of the size
    sizes[13] = 300
    turned[13, 7], cut[13, 0], cut[13, 7] = _flip(stored[12], 0), _flip(stored[12], 1), _flip(stored[12], 2, 63)
    # within the threshold, one bit in every band: 222's views against 455, 33 and 78
    turned[10, 3] = _flip(stored[2], 0, 16, 32, 48)
    cut[10, 0] = _flip(stored[3], 1, 17, 33, 49)
    cut[10, 2] = _flip(stored[5], 2, 18, 34, 50)
    files = [DuplicateFile(IDS[i], Path(f"lib/f{IDS[i]:04d}.png"), sizes[i], 100, 100, int(stored[i])) for i in range(N)]
    boxes = np.array([[i, i + 1, i + 40, i + 50] for i in range(N)], np.int32)
    return files, turned, cut, ok, has, boxes


FILES, TURNED, CUT, OK, HAS, BOXES = _inputs()


def _views_of_y(mode, y):
    whole = [(int(TURNED[y, k]), False, k) for k in range(1, 8)] if OK[y] else []
    crop = [(int(CUT[y, k]), True, k) for k in range(1, 8)] if HAS[y] else []
    return {"turned": whole, "trimmed": [(int(CUT[y, 0]), True, 0)] if HAS[y] else [], "turned_trimmed": whole + crop}[mode]


def _combinations(mode, ratio, banded=True):
    """Every (x, y, trimmed_x, trimmed_y, k, hamming) that counts; ``banded`` False: those within the threshold that share no band."""
    out = []
    for x in range(N):
        views_x = [(FILES[x].phash, False)] + ([(int(CUT[x, 0]), True)] if mode != "turned" and HAS[x] else [])
        for y in range(N):
            if x == y or FILES[x].file_id == FILES[y].file_id:
                continue
            small, large = sorted((FILES[x].size, FILES[y].size))
            if ratio and small > 0 and small / large < ratio:
                continue
            for hx, tx in views_x:
                for hy, ty, k in _views_of_y(mode, y):
                    d = bin(hx ^ hy).count("1")
                    shares = any((hx >> s) & 0xFFFF == (hy >> s) & 0xFFFF for s in (0, 16, 32, 48))
                    if d <= THRESHOLD and shares == banded:
                        out.append((x, y, tx, ty, k, d))
    return out


def _ordered(x, y, tx, ty, k, d):
    """(id pair, rank, (candidate a, candidate b)) with the smaller id first."""
    if FILES[x].file_id < FILES[y].file_id:
        return (FILES[x].file_id, FILES[y].file_id), (d, k, tx, ty), (x, y)
    return (FILES[y].file_id, FILES[x].file_id), (d, INVERSE[k], ty, tx), (y, x)


def _brute(mode, ratio):
    best = {}
    for combination in _combinations(mode, ratio):
        key, rank, who = _ordered(*combination)
        if key not in best or rank < best[key][0]:
            best[key] = (rank, who)
    box = lambda c, trimmed: tuple(int(v) for v in BOXES[c]) if trimmed else None
    out = []
    for (a, b), ((d, k, ta, tb), (ca, cb)) in sorted(best.items()):
        out.append({"turned": TurnedMatch(a, b, k, d), "trimmed": TrimmedMatch(a, b, ta, tb, d, box(ca, ta), box(cb, tb)),
                    "turned_trimmed": TransformedMatch(a, b, ta, tb, k, d, box(ca, ta), box(cb, tb))}[mode])
    return out


def _scanned(mode, ratio):
    scanner = DuplicateScanner(DuplicateScanConfig(hamming_threshold=THRESHOLD, size_ratio=ratio))
    if mode == "turned":
        return scanner.turned_edges(FILES, TURNED, OK)
    if mode == "trimmed":
        return scanner.trimmed_edges(FILES, CUT[:, 0], HAS, BOXES)
    return scanner.turned_trimmed_edges(FILES, TURNED, CUT, HAS, OK, BOXES)


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.delenv("KE_DUP_BUCKET_PAIR_CAP", raising=False)
    c = OracleScanContext()
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": c)
    return c


@pytest.mark.parametrize("ratio", [None, 0.5])
@pytest.mark.parametrize("mode", ["turned", "trimmed", "turned_trimmed"])
def test_the_one_scan_returns_what_the_docstrings_say(ctx, mode, ratio):
    want = _brute(mode, ratio)
    got = _scanned(mode, ratio)
    print(mode, ratio, *got, sep="\n  ")
    assert got == want
    assert len(ctx.calls) == 1 and all(m.file_id_a < m.file_id_b for m in got)


def _pairs(mode, ratio):
    return {(m.file_id_a, m.file_id_b) for m in _brute(mode, ratio)}


def _ranks(mode, pair):
    """The ordered ranks of every combination of a pair of ids, with the side each was found from."""
    return [(rank, FILES[x].file_id > FILES[y].file_id, k) for x, y, tx, ty, k, d in _combinations(mode, None)
            for key, rank, _ in [_ordered(x, y, tx, ty, k, d)] if key == pair]


@pytest.mark.parametrize("mode", ["turned", "turned_trimmed"])
def test_the_brute_force_holds_the_quarter_turns_found_from_the_larger_id(mode):
    for pair, raw_k in (((12, 907), 5), ((33, 455), 6)):
        found = _ranks(mode, pair)
        assert found and all(from_larger and k == raw_k for _, from_larger, k in found), (pair, found)
        match = next(m for m in _brute(mode, None) if (m.file_id_a, m.file_id_b) == pair)
        assert match.orientation == INVERSE[raw_k] != raw_k


@pytest.mark.parametrize("mode", ["turned", "turned_trimmed"])
def test_the_brute_force_holds_a_tie_on_hamming_between_two_orientations(mode):
    ranks = sorted(rank for rank, _, _ in _ranks(mode, (78, 810)))
    assert [r[:2] for r in ranks[:2]] == [(1, 2), (1, 3)]
    assert next(m for m in _brute(mode, None) if (m.file_id_a, m.file_id_b) == (78, 810)).orientation == 2


@pytest.mark.parametrize("mode, k", [("trimmed", 0), ("turned_trimmed", 4)])
def test_the_brute_force_holds_a_tie_on_hamming_and_orientation_between_the_flag_pairs(mode, k):
    ranks = sorted(rank for rank, _, _ in _ranks(mode, (64, 301)))
    assert ranks[:2] == [(1, k, False, True), (1, k, True, False)]
    match = next(m for m in _brute(mode, None) if (m.file_id_a, m.file_id_b) == (64, 301))
    assert (match.trimmed_a, match.trimmed_b) == (False, True)


def test_the_brute_force_holds_files_without_hashes_a_symmetric_picture_the_size_pair_and_the_bandless_pairs():
    assert not OK[8] and not HAS[9] and int(TURNED[8, 2]) == FILES[9].phash and int(CUT[9, 0]) == FILES[8].phash
    assert int(TURNED[11, 1]) == FILES[11].phash == int(CUT[11, 0]) and OK[11] and HAS[11]
    for mode in ("turned", "trimmed", "turned_trimmed"):
        pairs = _pairs(mode, None)
        assert (5, 590) not in pairs                                        # only through the rows that must not be read
        assert all(a != b for a, b in pairs) and not any(149 in p for p in pairs)
        assert (410, 700) in pairs and (410, 700) not in _pairs(mode, 0.5)
        assert pairs - _pairs(mode, 0.5) == {(410, 700)}
    # the stored hashes of the two files without rows still meet other files' views
    assert (222, 590) in _pairs("turned", None) and (5, 222) in _pairs("turned_trimmed", None)
    # four bits apart, one in every band: within the threshold, never a match
    for mode, other in (("turned", 455), ("trimmed", 33), ("turned_trimmed", 78)):
        bandless = {_ordered(*c)[0] for c in _combinations(mode, None, banded=False)}
        pair = tuple(sorted((222, other)))
        assert pair in bandless and pair not in _pairs(mode, None)
