"""Duplicate scanning on the MI355X: drop-in for the reference's ``dup.scanner``.

Same public surface as src/dup/scanner.py:430-436 -- ``DuplicateFile``, ``DuplicateCluster``,
``DuplicateClusterEntry``, ``DuplicateScanConfig``, ``DuplicateScanner`` -- so it plugs into
``DupViewModel(scanner_factory=...)`` (src/ui/viewmodels/dup_view_model.py:31,41).

Candidate generation (src/dup/scanner.py:227-299) runs as one all-pairs popcount scan on the
GPU (csrc/ke_scan.hip) with the closed form of the reference's bucket loop as predicate;
connected components come from the library's host union-find; keeper choice and every sort
key follow src/dup/scanner.py:320-356, 402-415.
"""
from __future__ import annotations

import gc
import logging
import math
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Iterable, Mapping, Optional, Sequence

import numpy as np

from . import _native

logger = logging.getLogger("dup.scanner")

_MASK64 = (1 << 64) - 1
_EXT_RANK = {"png": 4, "apng": 4, "webp": 3, "tiff": 2, "tif": 2, "bmp": 1, "gif": 1,
             "jpeg": 0, "jpg": 0, "jpe": 0, "jfif": 0}

PHASH_KEYS = ("phash_u64", "phash", "phash64", "phash_hex", "phash_bytes", "signature", "sig")


def _row_get(row, key, default=None):
    """Field of a dict / sqlite3.Row / attribute bag; malformed access yields the default."""
    try:
        if isinstance(row, dict):
            return row.get(key, default)
        keys = getattr(row, "keys", None)
        if keys is not None and key in keys():
            return row[key]
        return getattr(row, key, default)
    except (AttributeError, KeyError, TypeError):
        return default


def _parse_phash_any(raw) -> Optional[int]:
    """Any stored representation -> unsigned 64-bit int, or None (src/dup/scanner.py:44-81)."""
    if raw is None:
        return None
    if isinstance(raw, (bytes, bytearray, memoryview)):
        return int.from_bytes(bytes(raw), "big", signed=False) & _MASK64
    if isinstance(raw, str):
        text = raw.strip()
        if not text:
            return None
        for base in (0, 16):
            try:
                return int(text, base) & _MASK64
            except ValueError:
                continue
        return None
    try:
        return int(raw) & _MASK64
    except (OverflowError, TypeError, ValueError):
        return None


def _int_or_none(value):
    return int(value) if isinstance(value, (int, float)) else None


@dataclass(frozen=True)
class DuplicateFile:
    """What the scan needs to know about one file (src/dup/scanner.py:87-128)."""

    file_id: int
    path: Path
    size: Optional[int]
    width: Optional[int]
    height: Optional[int]
    phash: int
    embedding: Optional[tuple] = None

    @classmethod
    def from_row(cls, row: Mapping[str, object]) -> "DuplicateFile":
        raw = None
        for key in PHASH_KEYS:
            raw = _row_get(row, key)
            if raw is not None:
                break
        value = _parse_phash_any(raw)
        if value is None:
            raise ValueError("Row is missing perceptual hash information")
        return cls(
            file_id=int(_row_get(row, "file_id", _row_get(row, "id", -1))),
            path=Path(str(_row_get(row, "path", _row_get(row, "file_path", "")))),
            size=_int_or_none(_row_get(row, "size")),
            width=_int_or_none(_row_get(row, "width")),
            height=_int_or_none(_row_get(row, "height")),
            phash=value,
        )

    @property
    def resolution(self) -> int:
        return (self.width or 0) * (self.height or 0)

    @property
    def extension_priority(self) -> int:
        return _EXT_RANK.get(self.path.suffix.lower().lstrip("."), 0)


@dataclass(frozen=True)
class DuplicateClusterEntry:
    file: DuplicateFile
    best_hamming: Optional[int]


@dataclass(frozen=True)
class DuplicateCluster:
    files: list
    keeper_id: int


@dataclass(frozen=True)
class DuplicateScanConfig:
    """Thresholds of the scan; validation as src/dup/scanner.py:147-166.  ``exact`` (this project's, the last field so that
    the reference's positional constructor keeps working): every pair within ``hamming_threshold`` is an edge, whether or not
    it shares a band (``DuplicateScanner``'s docstring)."""

    hamming_threshold: int = 8
    size_ratio: Optional[float] = None
    band_bits: int = 16
    band_count: int = 4
    cosine_threshold: Optional[float] = None
    exact: bool = False

    def __post_init__(self) -> None:
        if self.band_bits <= 0:
            raise ValueError("band_bits must be positive")
        if self.band_count <= 0:
            raise ValueError("band_count must be positive")
        if not 0 <= self.hamming_threshold <= 64:
            raise ValueError("hamming_threshold must be in [0, 64]")
        if self.cosine_threshold is not None and not -1.0 <= self.cosine_threshold <= 1.0:
            raise ValueError("cosine_threshold must be between -1.0 and 1.0")


@dataclass
class DuplicateEdge:
    file_id_a: int
    file_id_b: int
    hamming: Optional[int]


@dataclass(frozen=True)
class TurnedMatch:
    """Two files of which one looks like a turned copy of the other: orientation ``orientation`` (turned.ORIENTATIONS) of
    file_id_b's picture is file_id_a's picture, to within ``hamming`` bits of the pHash.  file_id_a < file_id_b.  ``ssim``: the
    score of file a against that orientation of file b where the pair went through the SSIM re-check
    (api.find_turned_duplicates with ``ssim_threshold``), else None."""

    file_id_a: int
    file_id_b: int
    orientation: int
    hamming: int
    ssim: Optional[float] = None


@dataclass(frozen=True)
class TrimmedMatch:
    """Two files of which one looks like the other with a margin round it, to within ``hamming`` bits of the pHash.
    ``trimmed_a`` / ``trimmed_b``: whether that side entered the comparison cut to its content box; ``box_a`` / ``box_b``: that
    box as (x0, y0, x1, y1), None where the side is the file as it is.  file_id_a < file_id_b.  ``ssim``: the score of the two
    sides, each cut to its box where it is trimmed, where the pair went through the SSIM re-check
    (api.find_trimmed_duplicates with ``ssim_threshold``), else None."""

    file_id_a: int
    file_id_b: int
    trimmed_a: bool
    trimmed_b: bool
    hamming: int
    box_a: Optional[tuple] = None
    box_b: Optional[tuple] = None
    ssim: Optional[float] = None


@dataclass(frozen=True)
class TransformedMatch:
    """Two files of which one looks like a copy of the other that was given a margin, turned, or both: orientation
    ``orientation`` (turned.ORIENTATIONS) of file_id_b's picture -- cut to its content box first where ``trimmed_b`` -- is
    file_id_a's picture -- cut to its box where ``trimmed_a`` --, to within ``hamming`` bits of the pHash.  ``box_a`` / ``box_b``:
    that box as (x0, y0, x1, y1) on the file as it lies, None where the side is the whole file.  file_id_a < file_id_b.  ``ssim``:
    the score of the two views where the pair went through the SSIM re-check (api.find_turned_trimmed_duplicates with
    ``ssim_threshold``), else None."""

    file_id_a: int
    file_id_b: int
    trimmed_a: bool
    trimmed_b: bool
    orientation: int
    hamming: int
    box_a: Optional[tuple] = None
    box_b: Optional[tuple] = None
    ssim: Optional[float] = None


@dataclass(frozen=True)
class SimilarFile:
    """One neighbour of a query of ``DuplicateScanner.nearest``: a library file and the bits its pHash differs from the
    query's in."""

    file: DuplicateFile
    distance: int


@dataclass(frozen=True)
class _ViewTable:
    """The table of one view scan, one array entry per table entry: ``hashes`` u64[t]; ``row``, the candidate the entry is a
    view of; ``cut``, whether it is the hash of that candidate's content-box crop; ``k``, the orientation 0..7 it was turned
    by.  The scan compares the entries before ``first_new`` with those from it on, and with ``cross`` False the latter with
    each other as well (``Context.hamming_scan``)."""

    hashes: np.ndarray
    row: np.ndarray
    cut: np.ndarray
    k: np.ndarray
    first_new: int
    cross: bool

    @classmethod
    def of(cls, parts: Sequence[tuple], first: int, cross: bool) -> "_ViewTable":
        """``parts`` laid end to end, the first ``first`` of them before first_new.  A part is (hashes, candidate rows, cut):
        u64[m], orientation 0 of m candidates, or u64[m, 7], their orientations 1..7, candidate by candidate."""
        hashes, row, cut, k = [], [], [], []
        for part, rows, is_cut in parts:
            per = part.shape[1] if part.ndim == 2 else 1
            hashes.append(part.reshape(-1))
            row.append(np.repeat(np.asarray(rows, np.int64), per))
            cut.append(np.full(part.size, is_cut))
            k.append(np.tile(np.arange(1, 8), len(rows)) if per == 7 else np.zeros(len(rows), np.int64))
        return cls(np.concatenate(hashes), np.concatenate(row), np.concatenate(cut), np.concatenate(k),
                   sum(len(h) for h in hashes[:first]), cross)

    def edge(self, a: int, b: int) -> tuple:
        """An edge (a, b) of the scan -> (candidate a, trimmed_a, candidate b, trimmed_b, k)."""
        return int(self.row[a]), bool(self.cut[a]), int(self.row[b]), bool(self.cut[b]), int(self.k[b])


def _turned_table(stored, turned, src) -> _ViewTable:
    """[stored pHash of the n candidates | turned[i, 1:8] of the candidates ``src``, file by file], a cross scan."""
    return _ViewTable.of([(stored, np.arange(len(stored)), False), (turned[src, 1:8], src, False)], 1, True)


def _trimmed_table(stored, trimmed, src) -> _ViewTable:
    """[stored pHash of the n candidates | trimmed pHash of the candidates ``src``], a scan from first_new: trimmed x trimmed
    is compared as well."""
    return _ViewTable.of([(stored, np.arange(len(stored)), False), (trimmed[src], src, True)], 1, False)


def _turned_trimmed_table(stored, turned, cut, src_o, src_t) -> _ViewTable:
    """[stored pHash of the n candidates | cut[i, 0] of the candidates ``src_t``] against [turned[i, 1:8] of the candidates
    ``src_o`` | cut[i, 1:8] of ``src_t``], a cross scan."""
    return _ViewTable.of([(stored, np.arange(len(stored)), False), (cut[src_t, 0], src_t, True),
                          (turned[src_o, 1:8], src_o, False), (cut[src_t, 1:8], src_t, True)], 2, True)


def view_edge(a: int, b: int, n: int, trimmed_rows: Sequence[int], turned_rows: Sequence[int]) -> tuple:
    """An edge (a, b) of turned_trimmed_edges' table -> (candidate a, trimmed_a, candidate b, trimmed_b, k): the first part is
    [n stored pHashes | the trimmed pHash of candidates ``trimmed_rows``], the second [seven turned hashes of each of candidates
    ``turned_rows`` | seven turned hashes of the crop of each of ``trimmed_rows``]; a lies in the first part, b in the second."""
    blank = np.zeros((n, 8), np.uint64)
    table = _turned_trimmed_table(blank[:, 0], blank, blank, np.asarray(turned_rows, np.int64), np.asarray(trimmed_rows, np.int64))
    return table.edge(a, b)


def ordered_view(id_a: int, trimmed_a: bool, id_b: int, trimmed_b: bool, k: int) -> tuple:
    """(id_a, trimmed_a, id_b, trimmed_b, k) with the smaller id first: a match found from the file with the larger id has its
    flags exchanged and its orientation mapped through turned.INVERSE, so that k always turns b's view into a's."""
    from .turned import INVERSE

    if id_a > id_b:
        return id_b, trimmed_b, id_a, trimmed_a, INVERSE[k]
    return id_a, trimmed_a, id_b, trimmed_b, k


def view_rank(hamming: int, orientation: int, trimmed_a: bool, trimmed_b: bool) -> tuple:
    """What the one match kept per unordered pair of files is the smallest of."""
    return (int(hamming), int(orientation), bool(trimmed_a), bool(trimmed_b))


def _stored_hashes(candidates: Sequence[DuplicateFile]) -> np.ndarray:
    return np.fromiter((f.phash & _MASK64 for f in candidates), dtype=np.uint64, count=len(candidates))


def _ids_and_sizes(candidates: Sequence[DuplicateFile]) -> tuple:
    n = len(candidates)
    return (np.fromiter((f.file_id for f in candidates), dtype=np.int64, count=n),
            np.fromiter(((f.size or 0) for f in candidates), dtype=np.int64, count=n))


def _safe_positive_int(value: Optional[str]) -> Optional[int]:
    if value is None or not value.strip():
        return None
    try:
        parsed = int(value)
    except ValueError:
        return None
    return parsed if parsed > 0 else None


def _size_ok(size_a: int, size_b: int, ratio: float) -> bool:
    """src/dup/scanner.py:358-370."""
    if not ratio or ratio <= 0 or size_a <= 0 or size_b <= 0:
        return True
    smaller, larger = (size_a, size_b) if size_a < size_b else (size_b, size_a)
    return smaller / larger >= ratio


def _cosine(left: DuplicateFile, right: DuplicateFile) -> Optional[float]:
    """float64 cosine of two embeddings; None = "cannot tell, let it pass" (src/dup/scanner.py:383-400)."""
    u, v = left.embedding, right.embedding
    if u is None or v is None or len(u) == 0 or len(v) == 0 or len(u) != len(v):
        return None
    dot = sum(p * q for p, q in zip(u, v))
    nu, nv = math.sqrt(sum(p * p for p in u)), math.sqrt(sum(q * q for q in v))
    if nu == 0.0 or nv == 0.0:
        return None
    return dot / (nu * nv)


class DuplicateScanner:
    """GPU-backed replacement of the reference scanner (same constructor, same method).

    With ``config.exact`` every scan of this scanner -- ``candidate_edges`` and through it ``build_clusters`` and
    ``extend_clusters``, and the three view scans -- goes through ``ke_hamming_scan_exact``: an edge is every pair of the
    region within ``hamming_threshold`` whose ids differ and whose sizes pass ``size_ratio``; the band config only fills an
    edge's ``bands`` mask and decides nothing.  Under it
      * KE_DUP_BUCKET_PAIR_CAP is ignored (one INFO line says so; ``extend_clusters`` does not refuse it either): the cap is
        a property of buckets, and no bucket is walked;
      * the bucket statistics line is not logged;
      * with a file id that occurs twice, the edge kept per pair of ids is the one with the smallest (a, b): the reference's
        first-writer-wins order is an order of buckets, and a pair that shares none has no place in it;
      * ``last_counters`` counts pairs, not bucket pairs: ``pair_total`` is the region's pairs whose ids differ, worked out
        on the host from the id multiplicities (all shards together, as before); ``after_size`` is ``pair_total`` when no
        size ratio is set and None otherwise (nothing counts the pairs that pass the size filter alone; the log line prints
        n/a); ``after_ham`` is the device's edge count; ``after_cosine`` the edges that pass the cosine filter, one per pair
        where the banded funnel counts one per shared band -- so that it still equals ``after_ham`` when no cosine threshold
        is set; ``edges`` as ever."""

    def __init__(self, config: DuplicateScanConfig, *, device: int = 0, part_index: int = 0, part_count: int = 1) -> None:
        assert config.band_bits * config.band_count <= 64, "band config too large"
        self._config = config
        self._device = device
        self._part = (part_index, part_count)
        self._counters: Optional[dict] = None
        self._funnel: Optional[tuple] = None
        self._cap_noted = False

    # -- candidate edges ---------------------------------------------------------------------
    def _limits(self) -> tuple:
        """(size ratio, 0.0 = no size filter; KE_DUP_BUCKET_PAIR_CAP, None = no cap -- always None under ``exact``) of every
        scan of this scanner."""
        ratio = self._config.size_ratio
        cap = _safe_positive_int(os.environ.get("KE_DUP_BUCKET_PAIR_CAP"))
        if cap is not None and self._config.exact:
            if not self._cap_noted:
                logger.info("dup: exact scan, KE_DUP_BUCKET_PAIR_CAP=%d is ignored (no bucket is walked)", cap)
                self._cap_noted = True
            cap = None
        return (ratio if (ratio is not None and ratio > 0) else 0.0), cap

    def _scan(self, hashes, ids, sizes, **region) -> tuple:
        """(edges, counters) of ``Context.hamming_scan`` over one table under this scanner's config, limits and shard;
        ``region``: its first_new / cross."""
        cfg = self._config
        ratio, cap = self._limits()
        if cfg.exact:
            region = dict(region, exact=True)
        return _native.get_context(self._device).hamming_scan(
            hashes, len(hashes), ids=ids, sizes=sizes if ratio > 0 else None, threshold=cfg.hamming_threshold,
            band_bits=cfg.band_bits, band_count=cfg.band_count, size_ratio=ratio, bucket_pair_cap=cap or 0,
            part_index=self._part[0], part_count=self._part[1], **region)

    def candidate_edges(self, candidates: Sequence[DuplicateFile], first_new: int = 0) -> dict:
        """{(id_lo, id_hi): DuplicateEdge} exactly as the reference's ``edges`` dict ends up.  With ``first_new`` > 0 the
        candidates are [library | added] and only the pairs with a member at position >= first_new are scanned and
        returned (``ke_hamming_scan_from``): the pairs between two library files are not visited."""
        hashes, (ids, sizes) = _stored_hashes(candidates), _ids_and_sizes(candidates)
        ratio, cap = self._limits()
        if not self._config.exact:
            self._log_bucket_stats(hashes, cap)
        raw, counters = self._scan(hashes, ids, sizes, **({"first_new": int(first_new)} if first_new else {}))
        return self._edges_from_raw(candidates, hashes, ids, raw, counters, sizes=sizes, ratio=ratio, cap=cap, first_new=int(first_new))

    def _view_edges(self, candidates: Sequence[DuplicateFile], table: _ViewTable, boxes, make) -> list:
        """The one view scan: ``table``'s entries carry their candidate's id and size -- so the scan's own ``ids[i] != ids[j]``
        keeps a file from meeting a view of itself --, an edge decodes by lookup in the table, ``ordered_view`` puts the smaller
        id first, and per unordered pair of ids the match of the smallest ``view_rank`` is kept, the earlier edge at equal rank.
        Sorted by (id_a, id_b); ``make(id_a, id_b, trimmed_a, trimmed_b, orientation, hamming, box_a, box_b)`` builds a match."""
        base_ids, base_sizes = _ids_and_sizes(candidates)
        ids = base_ids[table.row]
        raw, _ = self._scan(table.hashes, ids, base_sizes[table.row], first_new=table.first_new, cross=table.cross)
        a, b = raw["a"], raw["b"]
        best: dict[tuple[int, int], tuple] = {}
        for id_a, t_a, c_a, id_b, t_b, c_b, k, h in zip(ids[a].tolist(), table.cut[a].tolist(), table.row[a].tolist(), ids[b].tolist(),
                                                        table.cut[b].tolist(), table.row[b].tolist(), table.k[b].tolist(), raw["h"].tolist()):
            if id_a > id_b:
                c_a, c_b = c_b, c_a
            id_a, t_a, id_b, t_b, k = ordered_view(id_a, t_a, id_b, t_b, k)
            rank = view_rank(h, k, t_a, t_b)
            if (id_a, id_b) not in best or rank < best[(id_a, id_b)][0]:
                best[(id_a, id_b)] = (rank, c_a, c_b)

        def box(c: int, trimmed: bool) -> Optional[tuple]:
            return tuple(int(v) for v in np.asarray(boxes)[c]) if trimmed and boxes is not None else None

        return [make(id_a, id_b, t_a, t_b, k, h, box(c_a, t_a), box(c_b, t_b)) for (id_a, id_b), ((h, k, t_a, t_b), c_a, c_b) in sorted(best.items())]

    def turned_edges(self, candidates: Sequence[DuplicateFile], turned, ok=None) -> list:
        """[TurnedMatch]: the pairs of files of which one looks like a mirrored, flipped or rotated copy of the other.

        ``turned``: u64[n, 8], row i the eight turned pHashes of candidates[i] (turned.turned_signatures; column 0 is not
        used, the stored pHash stands for the file as it is).  ``ok``: a mask of the rows that hold hashes; a file without
        takes part with its stored pHash only.  The table is [pHash of the n candidates | turned[i, 1:8] of the files
        with hashes, file by file], a turned entry carrying its source file's id and size -- the scan's own ``ids[i] !=
        ids[j]`` therefore drops a symmetric picture matching itself -- and the scan is a cross scan with first_new = n
        (``ke_hamming_scan_cross``): the 7 n turned entries are not compared with each other.  An edge (a, b) is file a
        against the orientation and the file that entry b of the table carries (``_ViewTable``).  One match is kept per
        unordered pair of files: the smallest hamming, then the smallest orientation (``view_rank``).  A match found from the
        file with the larger id has its orientation mapped through turned.INVERSE (``ordered_view``), so that ``orientation``
        always turns b's picture into a's.  size_ratio, the band config, KE_DUP_BUCKET_PAIR_CAP and this scanner's part_index /
        part_count apply as in ``candidate_edges``; the funnel counters are not touched."""
        n = len(candidates)
        turned = np.asarray(turned, dtype=np.uint64).reshape(n, 8)
        src = np.arange(n) if ok is None else np.nonzero(np.asarray(ok, bool))[0]
        if n == 0 or len(src) == 0:
            return []
        return self._view_edges(candidates, _turned_table(_stored_hashes(candidates), turned, src), None,
                                lambda a, b, t_a, t_b, k, h, box_a, box_b: TurnedMatch(a, b, k, h))

    def trimmed_edges(self, candidates: Sequence[DuplicateFile], hashes, has, boxes=None) -> list:
        """[TrimmedMatch]: the pairs of files of which one looks like the other with a margin round it.

        ``hashes``: u64[n], entry i the trimmed pHash of candidates[i]; ``has``: the mask of the files that have one
        (trimmed.trimmed_signatures); ``boxes``: int32[n, 4], the boxes the matches carry (None: a trimmed side carries no
        box either).  The table is [stored pHash of the n candidates | trimmed hash of the files with one], a trimmed entry
        carrying its file's id and size -- the scan's own ``ids[i] != ids[j]`` therefore drops a file against its own crop --
        and the scan is the scan from first_new = n (``ke_hamming_scan_from``), NOT the cross scan: two copies of a picture
        with different margins meet in trimmed x trimmed.  One match is kept per unordered pair of files: the smallest
        hamming, then (trimmed_a, trimmed_b) in order (``view_rank``).  size_ratio, the band config, KE_DUP_BUCKET_PAIR_CAP and
        this scanner's part_index / part_count apply as in ``candidate_edges``; the funnel counters are not touched."""
        n = len(candidates)
        hashes = np.asarray(hashes, dtype=np.uint64).reshape(n)
        src = np.nonzero(np.asarray(has, bool).reshape(n))[0]
        if n == 0 or len(src) == 0:
            return []
        return self._view_edges(candidates, _trimmed_table(_stored_hashes(candidates), hashes, src), boxes,
                                lambda a, b, t_a, t_b, k, h, box_a, box_b: TrimmedMatch(a, b, t_a, t_b, h, box_a, box_b))

    def turned_trimmed_edges(self, candidates: Sequence[DuplicateFile], turned, trimmed_turned, has, ok=None, boxes=None) -> list:
        """[TransformedMatch] of orientation 1..7: the pairs of files of which one looks like a turned copy of the other, either
        side whole or cut to its content box -- a scan laid on the glass sideways with a white margin, a letterboxed frame that
        was mirrored.

        ``turned``: u64[n, 8], the turned pHashes of candidates[i]; ``ok``: the rows that hold them.  ``trimmed_turned``: u64[n, 8],
        the turned pHashes of the crop; ``has``: the files whose box qualifies; ``boxes``: int32[n, 4], the boxes the matches carry
        (all from turned_trimmed.turned_trimmed_signatures).  One cross scan (``ke_hamming_scan_cross``) whose first_new is the
        length of the first part: [stored pHash of the n candidates | trimmed pHash (column 0) of the m files with one] against
        [turned[:, 1:8] of the files with hashes | trimmed_turned[:, 1:8] of the m files]; neither part is compared with itself.
        Every entry carries its file's id and size, so a file never meets itself, and size_ratio, the band config,
        KE_DUP_BUCKET_PAIR_CAP and this scanner's part_index / part_count apply as in ``turned_edges``.  An edge decodes to (a's
        side trimmed or not, b's side trimmed or not, k) (``view_edge``); found from the file with the larger id, the flags are
        exchanged and k goes through turned.INVERSE (``ordered_view``), so that ``orientation`` always turns b's (cut) picture
        into a's (cut) picture.  One match is kept per unordered pair of files: the smallest (hamming, orientation, trimmed_a,
        trimmed_b).  Orientation 0 is not in the table: those pairs are ``candidate_edges``' and ``trimmed_edges``'."""
        n = len(candidates)
        turned = np.asarray(turned, dtype=np.uint64).reshape(n, 8)
        cut = np.asarray(trimmed_turned, dtype=np.uint64).reshape(n, 8)
        src_o = np.arange(n) if ok is None else np.nonzero(np.asarray(ok, bool).reshape(n))[0]
        src_t = np.nonzero(np.asarray(has, bool).reshape(n))[0]
        if n == 0 or len(src_o) + len(src_t) == 0:
            return []
        return self._view_edges(candidates, _turned_trimmed_table(_stored_hashes(candidates), turned, cut, src_o, src_t), boxes,
                                TransformedMatch)

    # -- the reference's funnel counters (src/dup/scanner.py:258-299) ---------------------------------------------
    def _band_values(self, hashes: np.ndarray, band: int) -> np.ndarray:
        cfg = self._config
        mask = np.uint64((1 << cfg.band_bits) - 1) if cfg.band_bits < 64 else np.uint64(_MASK64)
        return (hashes >> np.uint64(band * cfg.band_bits)) & mask

    def _same_id_bucket_pairs(self, hashes, ids, sizes, ratio, cap) -> tuple[int, int]:
        """Bucket pairs of equal file id (the reference skips them before counting, :266): (all, those passing the
        size filter).  Only ids that occur more than once are looked at."""
        uniq, inverse, counts = np.unique(ids, return_inverse=True, return_counts=True)
        if not (counts > 1).any():
            return 0, 0
        cfg = self._config
        total = sized = 0
        bucket_len = []
        for band in range(cfg.band_count):
            vals = self._band_values(hashes, band)
            _, inv, cnt = np.unique(vals, return_inverse=True, return_counts=True)
            bucket_len.append((vals, cnt[inv]))
        for g in np.nonzero(counts > 1)[0]:
            pos = np.nonzero(inverse == g)[0]
            for x in range(len(pos) - 1):
                for y in range(x + 1, len(pos)):
                    i, j = int(pos[x]), int(pos[y])
                    for vals, blen in bucket_len:
                        if vals[i] != vals[j]:
                            continue
                        length = int(blen[i])
                        if cap is not None and length * (length - 1) // 2 > cap:
                            continue
                        total += 1
                        sized += _size_ok(int(sizes[i]), int(sizes[j]), ratio)
        return total, sized

    def _edges_from_raw(self, candidates, hashes, ids, raw, counters, *, sizes=None, ratio=0.0, cap=None, first_new=0) -> dict:
        cfg = self._config
        order = np.lexsort((raw["b"], raw["a"]))
        raw = raw[order]
        after_cos = 0
        keyed: dict[tuple[int, int], list] = {}
        for a, b, h, bands in zip(raw["a"].tolist(), raw["b"].tolist(), raw["h"].tolist(), raw["bands"].tolist()):
            if cfg.cosine_threshold is not None:
                cos = _cosine(candidates[a], candidates[b])
                if cos is not None and cos < cfg.cosine_threshold:
                    continue
            after_cos += 1 if cfg.exact else bin(bands & 0xFFFFFFFF).count("1")
            ia, ib = int(ids[a]), int(ids[b])
            keyed.setdefault((ia, ib) if ia < ib else (ib, ia), []).append((a, b, h, bands))
        edges: dict[tuple[int, int], DuplicateEdge] = {}
        first_idx_cache: dict[tuple[int, int], int] = {}
        mask = (1 << cfg.band_bits) - 1

        def bucket_rank(pos: int, bands: int) -> int:
            # dict insertion order of the reference's buckets: (first position holding the value, band)
            best = None
            for band in range(min(cfg.band_count, 32)):
                if not (bands >> band) & 1:
                    continue
                val = (int(hashes[pos]) >> (band * cfg.band_bits)) & mask
                key = (band, val)
                if key not in first_idx_cache:
                    col = (hashes >> np.uint64(band * cfg.band_bits)) & np.uint64(mask)
                    first_idx_cache[key] = int(np.argmax(col == np.uint64(val)))
                rank = first_idx_cache[key] * cfg.band_count + band
                best = rank if best is None or rank < best else best
            return best if best is not None else 0

        for key, hits in keyed.items():
            if len(hits) > 1 and cfg.exact:  # duplicate file ids under exact: no bucket order to go by, the smallest (a, b)
                hits.sort(key=lambda t: (t[0], t[1]))
            elif len(hits) > 1:  # duplicate file ids: the first writer wins (src/dup/scanner.py:287-290)
                hits.sort(key=lambda t: (bucket_rank(t[0], t[3]), t[0], t[1]))
            a, b, h, _ = hits[0]
            edges[key] = DuplicateEdge(int(ids[a]), int(ids[b]), int(h))
        # The reference's funnel figures (src/dup/scanner.py:292-299) are a log line, not part of the result: they are worked
        # out when somebody looks -- the logger at INFO, or a reader of ``last_counters`` -- and cost nothing otherwise.
        self._counters = None
        self._funnel = (hashes, ids, sizes, ratio, cap, [int(c) for c in counters], after_cos, len(edges), first_new)
        if logger.isEnabledFor(logging.INFO):
            c = self.last_counters
            logger.info("dup: pairs total=%d -> size=%s -> ham=%d -> cosine=%d -> edges=%d", c["pair_total"],
                        "n/a" if c["after_size"] is None else c["after_size"], c["after_ham"], c["after_cosine"], c["edges"])
        return edges

    @staticmethod
    def _region_pairs_of_differing_ids(ids: np.ndarray, first_new: int) -> int:
        """Pairs i < j with j >= first_new and ids[i] != ids[j]: the region's pairs less, per id, the pairs among its
        occurrences that lie in the region."""
        n, f = len(ids), int(first_new)
        total = n * (n - 1) // 2 - f * (f - 1) // 2
        uniq, inverse, counts = np.unique(ids, return_inverse=True, return_counts=True)
        if (counts > 1).any():
            old = np.bincount(inverse[:f], minlength=len(uniq)).astype(object)
            counts = counts.astype(object)
            total -= int((counts * (counts - 1) // 2 - old * (old - 1) // 2).sum())
        return total

    @property
    def last_counters(self) -> Optional[dict]:
        """The funnel of the last scan: "pairs total" = the device's bucket-pair count (band histograms) minus bucket pairs of
        equal file id; "size" = the same with the size filter (``ke_band_pairs_after_size``).  A shard reports the whole
        table's figures for these two (they do not depend on the tiles it was dealt), its own share for the rest.
        After ``candidate_edges(..., first_new)`` the same split holds for the region: ``pairs_evaluated``, ``after_ham``,
        ``after_cosine`` and ``edges`` are taken over the pairs with a member at position >= first_new, ``pair_total`` and
        ``after_size`` remain the whole table's (bucket sizes are a property of the table, not of the region).
        Under ``config.exact`` the keys count pairs of the region instead (the class docstring)."""
        if self._counters is None and self._funnel is not None:
            hashes, ids, sizes, ratio, cap, counters, after_cos, n_edges, first_new = self._funnel
            if self._config.exact:
                pair_total = self._region_pairs_of_differing_ids(ids, first_new)
                self._counters = {"pairs_evaluated": counters[0], "pair_total": pair_total,
                                  "after_size": pair_total if not (ratio > 0 and sizes is not None) else None,
                                  "after_ham": counters[2], "after_cosine": after_cos, "edges": n_edges}
                self._funnel = None
                return self._counters
            same_total, same_sized = self._same_id_bucket_pairs(hashes, ids, sizes if sizes is not None else np.zeros(len(ids), np.int64),
                                                                ratio, cap)
            pair_total = counters[3] - same_total
            if ratio > 0 and sizes is not None:
                cfg = self._config
                after_size = _native.get_context(self._device).band_pairs_after_size(
                    hashes, sizes, len(hashes), band_bits=cfg.band_bits, band_count=cfg.band_count, size_ratio=ratio,
                    bucket_pair_cap=cap or 0) - same_sized
            else:
                after_size = pair_total
            self._counters = {"pairs_evaluated": counters[0], "pair_total": pair_total, "after_size": after_size,
                              "after_ham": counters[1], "after_cosine": after_cos, "edges": n_edges}
            self._funnel = None
        return self._counters

    @last_counters.setter
    def last_counters(self, value: Optional[dict]) -> None:
        self._counters, self._funnel = value, None

    def _log_bucket_stats(self, hashes: np.ndarray, cap: Optional[int]) -> None:
        if not logger.isEnabledFor(logging.INFO) and cap is None:
            return
        cfg = self._config
        mask = np.uint64((1 << cfg.band_bits) - 1)
        n_buckets = ge2 = max_bucket = 0
        for band in range(cfg.band_count):
            _, counts = np.unique((hashes >> np.uint64(band * cfg.band_bits)) & mask, return_counts=True)
            n_buckets += len(counts)
            ge2 += int((counts >= 2).sum())
            max_bucket = max(max_bucket, int(counts.max()) if len(counts) else 0)
        max_pairs = max_bucket * (max_bucket - 1) // 2
        logger.info("dup: buckets=%d (>=2:%d) max_bucket=%d max_bucket_pairs=%d pair_cap=%s", n_buckets, ge2, max_bucket,
                    max_pairs, cap)
        if cap is not None and max_pairs > cap:
            logger.warning("dup: largest bucket has %d pair(s), above KE_DUP_BUCKET_PAIR_CAP=%d; large buckets will be skipped",
                           max_pairs, cap)

    # -- the seam ----------------------------------------------------------------------------
    def build_clusters(self, files: Iterable[DuplicateFile]) -> list:
        cfg = self._config
        candidates = [f for f in files if f.phash is not None]
        logger.info("dup: candidates=%d band_bits=%d band_count=%d ham_th=%d size_ratio=%s cosine_th=%s", len(candidates),
                    cfg.band_bits, cfg.band_count, cfg.hamming_threshold, cfg.size_ratio, cfg.cosine_threshold)
        if len(candidates) < 2:
            return []
        # The host part allocates a few objects per edge and per cluster and none of them is part of a reference cycle; with a
        # million DuplicateFile objects alive every full pass of the cycle collector it sets off walks all of them (1.3 of the
        # 1.7 s of a million-file call went there).  The collector is paused for the duration of the call.
        paused = gc.isenabled()
        gc.disable()
        try:
            edges = self.candidate_edges(candidates)
            if not edges:
                return []
            return assemble_clusters(candidates, edges.values())
        finally:
            if paused:
                gc.enable()

    def extend_clusters(self, library: Iterable[DuplicateFile], added: Iterable[DuplicateFile], previous: Iterable[DuplicateCluster]) -> list:
        """The clusters of ``build_clusters(list(library) + list(added))`` -- membership, order, keepers and best_hamming
        -- from ``previous`` = what ``build_clusters(library)`` returned under the same config, and a scan of only the
        pairs that touch an added file.  Connectivity among library files comes from ``previous``' memberships, an old
        member's best_hamming is the minimum of its previous value and its new edges.

        ValueError where that equality cannot hold: with KE_DUP_BUCKET_PAIR_CAP set and not ``config.exact`` (buckets grow with the table, so an
        edge between two library files can vanish under the cap and ``previous`` would keep it), with a file id that
        occurs twice across library + added (the first-writer-wins rule between equal ids needs the pairs this scan leaves
        out), and when ``previous`` names a file that is not in ``library``."""
        cfg = self._config
        if self._limits()[1] is not None:
            raise ValueError("extend_clusters: KE_DUP_BUCKET_PAIR_CAP is set; under a bucket pair cap edges between library "
                             "files can disappear as the table grows, so previous clusters cannot be extended")
        old = [f for f in library if f.phash is not None]
        new = [f for f in added if f.phash is not None]
        candidates = old + new
        previous = list(previous)
        seen: set = set()
        for f in candidates:
            if f.file_id in seen:
                raise ValueError(f"extend_clusters: file id {f.file_id} occurs twice across library + added")
            seen.add(f.file_id)
        old_ids = {f.file_id for f in old}
        for cluster in previous:
            for entry in cluster.files:
                if entry.file.file_id not in old_ids:
                    raise ValueError(f"extend_clusters: previous names file id {entry.file.file_id}, which is not in library")
        logger.info("dup: extend library=%d added=%d previous_clusters=%d ham_th=%d", len(old), len(new), len(previous),
                    cfg.hamming_threshold)
        if len(candidates) < 2:
            return []
        paused = gc.isenabled()
        gc.disable()
        try:
            edges = self.candidate_edges(candidates, first_new=len(old)) if new and old else \
                self.candidate_edges(candidates) if new else {}
            return assemble_clusters(candidates, edges.values(), previous=previous)
        finally:
            if paused:
                gc.enable()

    def nearest(self, library: Iterable[DuplicateFile], queries: Iterable[DuplicateFile], k: int,
                max_distance: Optional[int] = None) -> list:
        """One list per query of at most ``k`` ``SimilarFile(file, distance)``: the library files whose pHash lies nearest the
        query's, best first -- by distance, then by the file's place in ``library`` (``ke_hamming_nearest``).

        This is a ranking by Hamming distance ALONE.  It does not read ``hamming_threshold``, the band config, ``size_ratio``
        or ``cosine_threshold`` from the scanner's config: a pair that shares no 16-bit band, which ``build_clusters`` cannot
        link, is found here.  ``max_distance``: leave out library files further away than this; None means 64, no limit.
        Library files without a pHash are left out; a query without one gets [].  A query whose ``file_id`` is a real id (not
        None, not negative) never gets the library files with that id -- itself, when it comes from the library -- but does
        get another file with the same hash; a query without an id excludes nothing.  ``k`` may exceed the library: a row
        is as long as there are files within ``max_distance``.  ``k`` is at most 1024 (KE_NEAREST_MAX_K)."""
        files = [f for f in library if f.phash is not None]
        queries = list(queries)
        out: list = [[] for _ in queries]
        asked = [i for i, q in enumerate(queries) if q.phash is not None]
        if not files or not asked:
            return out
        hashes = np.fromiter((f.phash & _MASK64 for f in files), dtype=np.uint64, count=len(files))
        q_hashes = np.fromiter((queries[i].phash & _MASK64 for i in asked), dtype=np.uint64, count=len(asked))
        # the kernel's id rule on codes of this call's own: a real file id -> its first position in the library; a library file
        # without an id (-2) and a query without one or with one the library does not hold (-1) match nothing
        code: dict = {}
        ids = np.empty(len(files), np.int64)
        for at, f in enumerate(files):
            ids[at] = code.setdefault(f.file_id, at) if _has_id(f) else -2
        q_ids = np.fromiter((code.get(queries[i].file_id, -1) if _has_id(queries[i]) else -1 for i in asked), dtype=np.int64,
                            count=len(asked))
        ctx = _native.get_context(self._device)
        index, distance, count, _within = ctx.hamming_nearest(hashes, q_hashes, k=int(k), max_distance=64 if max_distance is None else int(max_distance),
                                                              ids=ids, query_ids=q_ids)
        for row, i in enumerate(asked):
            c = int(count[row])
            out[i] = [SimilarFile(files[p], d) for p, d in zip(index[row, :c].tolist(), distance[row, :c].tolist())]
        return out

    @staticmethod
    def _choose_keeper(entries: Sequence[DuplicateClusterEntry]) -> int:
        return min(entries, key=_keeper_key).file.file_id


def _has_id(f: DuplicateFile) -> bool:
    """A file id that names a file: ``from_row`` gives -1 to a row without one."""
    return f.file_id is not None and f.file_id >= 0


def _keeper_key(entry: DuplicateClusterEntry) -> tuple:
    f = entry.file
    return (-(f.size or 0), -f.resolution, -f.extension_priority, f.path.suffix.lower(), f.path.name.lower(), f.file_id)


def _file_keys(f: DuplicateFile) -> tuple:
    """(keeper key, entry sort key without the keeper flag) of src/dup/scanner.py:402-415 and :338-347."""
    suffix = f.path.suffix.lower()
    name = f.path.name.lower()
    head = (-(f.size or 0), -f.resolution, -_EXT_RANK.get(suffix.lstrip("."), 0))
    return head + (suffix, name, f.file_id), head + (name, f.file_id)


def assemble_clusters(candidates: Sequence[DuplicateFile], edges: Iterable[DuplicateEdge], previous: Sequence[DuplicateCluster] = ()) -> list:
    """Edges -> ordered clusters (src/dup/scanner.py:304-356).  Components come from the library's host union-find over
    compacted file ids; best_hamming and the grouping are array work, Python only touches the members of each cluster once
    (a million-file table leaves some 60 000 clusters: their keys, not the union-find, are the time).

    ``previous``: clusters of an earlier call over a part of ``candidates`` whose edges are not among ``edges``
    (``extend_clusters``).  Each stands in for its edges: its members are linked (to its first member, without a
    distance) and each member's best_hamming starts from the value it had there."""
    edges = list(edges)
    carried = [(e.file.file_id, e.best_hamming) for c in previous if len(c.files) > 1 for e in c.files]
    for c in previous:
        head = c.files[0].file.file_id
        edges.extend(DuplicateEdge(head, e.file.file_id, None) for e in c.files[1:])
    if not edges:
        return []
    m = len(edges)
    by_id = {f.file_id: f for f in candidates}          # later duplicates of an id win, as in the reference
    ends = np.empty(2 * m, np.int64)
    ends[:m] = np.fromiter((e.file_id_a for e in edges), np.int64, m)
    ends[m:] = np.fromiter((e.file_id_b for e in edges), np.int64, m)
    ham = np.fromiter((-1 if e.hamming is None else e.hamming for e in edges), np.int64, m)
    node_ids, inverse = np.unique(ends, return_inverse=True)         # ascending ids -> members ascending
    raw = np.zeros(m, _native.EDGE_DTYPE)
    raw["a"], raw["b"] = inverse[:m], inverse[m:]
    labels = _native.cluster_labels(raw, len(node_ids))
    none = np.iinfo(np.int64).max
    best = np.full(len(node_ids), none, np.int64)
    known = ham >= 0
    np.minimum.at(best, inverse[:m][known], ham[known])
    np.minimum.at(best, inverse[m:][known], ham[known])
    carried = [(i, b) for i, b in carried if b is not None]
    if carried:
        at = np.searchsorted(node_ids, np.fromiter((i for i, _ in carried), np.int64, len(carried)))
        np.minimum.at(best, at, np.fromiter((b for _, b in carried), np.int64, len(carried)))
    order = np.argsort(labels, kind="stable")
    sorted_labels = labels[order]
    cuts = np.nonzero(np.concatenate(([True], sorted_labels[1:] != sorted_labels[:-1], [True])))[0].tolist()
    member_ids = node_ids[order].tolist()
    member_best = best[order].tolist()
    ranked = []                                          # (cluster sort key, cluster)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi - lo < 2:
            continue
        members = [(by_id.get(member_ids[k]), member_best[k]) for k in range(lo, hi)]
        members = [(f, None if b == none else b) for f, b in members if f is not None]
        if len(members) < 2:
            continue
        if len(members) == 2 and (members[0][0].size or 0) != (members[1][0].size or 0):
            # the common case needs no key at all: two files of different size, the larger is the keeper and comes first
            if (members[0][0].size or 0) < (members[1][0].size or 0):
                members.reverse()
            keeper = members[0][0].file_id
        else:
            keyed = [(_file_keys(f), f, b) for f, b in members]
            keeper = min(keyed, key=lambda t: t[0][0])[1].file_id
            keyed.sort(key=lambda t: (0 if t[1].file_id == keeper else 1,) + t[0][1])
            members = [(f, b) for _, f, b in keyed]
        entries = [DuplicateClusterEntry(f, b) for f, b in members]
        top = max((f.size or 0) for f, _ in members)
        ranked.append(((-top, members[0][0].path.as_posix().lower()), DuplicateCluster(files=entries, keeper_id=keeper)))
    ranked.sort(key=lambda t: t[0])
    return [c for _, c in ranked]


__all__ = ["DuplicateFile", "DuplicateCluster", "DuplicateClusterEntry", "DuplicateScanConfig", "DuplicateScanner"]
