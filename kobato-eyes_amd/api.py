"""The two names the north star asks for -- ``compute_signature()`` / ``find_duplicates()`` --
as thin aliases over the drop-ins of the reference's real seams (SURVEY finding 2), plus a
headless restatement of the production call sequence ``DuplicateScanRunnable.run``
(src/ui/dup_workers.py:148-239): rows -> fill missing hashes -> from_row (bad rows skipped)
-> build_clusters.  Config surface: ``{hamming_threshold, ssim_threshold}`` with the defaults
and coercions of PipelineSettings (src/core/config/schema.py:116-117, 186-201).
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, Iterable, Mapping, Optional, Sequence

import importlib

from . import fastsig, refine as _refine

_phash = importlib.import_module(".phash", __package__)   # the package also exports a function named phash
from .cluster import ClusterBuilder
from .scanner import DuplicateCluster, DuplicateFile, DuplicateScanConfig, DuplicateScanner, SimilarFile

logger = logging.getLogger(__name__)


@dataclass(frozen=True)
class DedupSettings:
    """``hamming_threshold`` / ``ssim_threshold`` as persisted by the reference's settings file."""

    hamming_threshold: int = 10
    ssim_threshold: float = 0.92

    @staticmethod
    def coerce(hamming_threshold=None, ssim_threshold=None) -> "DedupSettings":
        try:
            ham = max(0, int(hamming_threshold))
        except (TypeError, ValueError):
            ham = 10
        try:
            ssim = float(ssim_threshold)
        except (TypeError, ValueError):
            ssim = 0.92
        return DedupSettings(ham, ssim)


def compute_signature(image_or_path, *, device: int = 0) -> tuple[int, int]:
    """(signed pHash, signed dHash) of a PIL image, ndarray or file path."""
    if isinstance(image_or_path, (str, Path)):
        from PIL import Image

        with Image.open(image_or_path) as im:
            return _phash.phash_dhash(im, device=device)
    return _phash.phash_dhash(image_or_path, device=device)


def _parse_files(files: Iterable) -> list:
    """DuplicateFile objects or row mappings -> DuplicateFile objects; malformed rows are skipped (src/ui/dup_workers.py:205-209)."""
    parsed: list[DuplicateFile] = []
    for item in files:
        if isinstance(item, DuplicateFile):
            parsed.append(item)
            continue
        try:
            parsed.append(DuplicateFile.from_row(item))
        except ValueError:
            logger.debug("skipping row without a usable hash")
    return parsed


def _make_scanner(scanner_factory, config: DuplicateScanConfig, device: int):
    try:
        return scanner_factory(config, device=device)         # one process per GPU: scan on the caller's device
    except TypeError:
        return scanner_factory(config)                        # a foreign factory with the reference's one-argument signature


def _ssim_kept(edges: list, candidates: Sequence[DuplicateFile], ssim_threshold: float, device: int, devices) -> list:
    """The edges whose two files pass the SSIM re-check: every file decoded once, one fit + one SSIM launch per size group
    (refine_pairs), not one of each per edge."""
    by_id = {f.file_id: f for f in candidates}
    matches = _refine.refine_pairs([(e.file_id_a, e.file_id_b, by_id[e.file_id_a].path, by_id[e.file_id_b].path) for e in edges],
                                   thresholds=_refine.RefinementThresholds(ssim=ssim_threshold), device=device, devices=devices)
    return [e for e, m in zip(edges, matches) if m is not None and m.is_duplicate]


def find_duplicates(files: Iterable, *, hamming_threshold: int = 8, ssim_threshold: Optional[float] = None,
                    size_ratio: Optional[float] = None, band_bits: int = 16, band_count: int = 4,
                    scanner_factory: Callable[[DuplicateScanConfig], DuplicateScanner] = DuplicateScanner,
                    device: Optional[int] = None, devices: Optional[Sequence[int]] = None, exact: bool = False) -> list:
    """Clusters of near-duplicates.

    ``files``: DuplicateFile objects or row mappings (anything ``DuplicateFile.from_row`` takes;
    malformed rows are skipped as at src/ui/dup_workers.py:205-209).  With ``ssim_threshold``
    set, every candidate edge is re-checked with the SSIM kernel on the files' pixels and only
    edges with ``ssim >= ssim_threshold`` survive into the clusters.  ``devices``: the SSIM re-check is spread over one worker
    process per entry (``refine_pairs``); the scan stays in this process, on ``device`` (default ``devices[0]``, else 0).
    ``exact``: every pair within ``hamming_threshold`` is a candidate edge, whether or not it shares a band
    (``DuplicateScanConfig.exact``; ``DuplicateScanner`` says what else changes under it).
    """
    if device is None:
        device = int(devices[0]) if devices else 0
    parsed = _parse_files(files)
    config = DuplicateScanConfig(hamming_threshold=hamming_threshold, size_ratio=size_ratio, band_bits=band_bits,
                                 band_count=band_count, exact=bool(exact))
    scanner = _make_scanner(scanner_factory, config, device)
    if ssim_threshold is None:
        return scanner.build_clusters(parsed)
    from .scanner import assemble_clusters

    candidates = [f for f in parsed if f.phash is not None]
    if len(candidates) < 2:
        return []
    edges = list(scanner.candidate_edges(candidates).values())
    kept = _ssim_kept(edges, candidates, ssim_threshold, device, devices)
    return assemble_clusters(candidates, kept) if kept else []


def find_new_duplicates(library: Iterable, added: Iterable, *, previous: Optional[Sequence[DuplicateCluster]] = None,
                        hamming_threshold: int = 8, ssim_threshold: Optional[float] = None, size_ratio: Optional[float] = None,
                        band_bits: int = 16, band_count: int = 4,
                        scanner_factory: Callable[[DuplicateScanConfig], DuplicateScanner] = DuplicateScanner,
                        device: Optional[int] = None, devices: Optional[Sequence[int]] = None, exact: bool = False) -> list:
    """The clusters that contain at least one file of ``added``, from a scan of only the pairs that touch an added file:
    the pairs between two ``library`` files, which an earlier run judged, are neither scanned nor re-checked.

    ``library`` / ``added``: as ``files`` of ``find_duplicates``.  ``previous``: the clusters an earlier
    ``find_duplicates(library, ...)`` returned under the same thresholds.  With it and without ``ssim_threshold`` the
    result equals the clusters of ``find_duplicates(library + added, ...)`` that contain an added file
    (``DuplicateScanner.extend_clusters``, which also says when it raises ValueError).  With ``ssim_threshold`` only the
    new edges go to ``refine_pairs``; ``previous``' memberships stand for the library's own edges as they are, so they
    should come from a run with the same ``ssim_threshold``.  Without ``previous`` the clusters are assembled from the
    new edges alone: a link between two library files is then absent, so two library files appear together only when an
    added file (or a chain of them) connects them, and a library member's best_hamming is taken over its new edges only.
    ``exact``: as for ``find_duplicates``; ``previous`` should then come from an exact run as well.
    """
    if device is None:
        device = int(devices[0]) if devices else 0
    old, new = _parse_files(library), _parse_files(added)
    config = DuplicateScanConfig(hamming_threshold=hamming_threshold, size_ratio=size_ratio, band_bits=band_bits,
                                 band_count=band_count, exact=bool(exact))
    scanner = _make_scanner(scanner_factory, config, device)
    from .scanner import assemble_clusters

    if previous is not None and ssim_threshold is None:
        clusters = scanner.extend_clusters(old, new, previous)
    else:
        old = [f for f in old if f.phash is not None]
        new = [f for f in new if f.phash is not None]
        candidates = old + new
        if not new or len(candidates) < 2:
            return []
        edges = list(scanner.candidate_edges(candidates, first_new=len(old)).values())
        if ssim_threshold is not None and edges:
            edges = _ssim_kept(edges, candidates, ssim_threshold, device, devices)
        clusters = assemble_clusters(candidates, edges, previous=previous or ())
    new_ids = {f.file_id for f in new}
    return [c for c in clusters if any(e.file.file_id in new_ids for e in c.files)]


def _parse_query(item, device: int) -> DuplicateFile:
    """A query of ``find_similar`` -> a DuplicateFile; one without a usable hash keeps its place with ``phash`` None."""
    if isinstance(item, DuplicateFile):
        return item
    if isinstance(item, (str, Path)):
        return DuplicateFile(file_id=-1, path=Path(item), size=None, width=None, height=None,
                             phash=compute_signature(item, device=device)[0] & ((1 << 64) - 1))
    if isinstance(item, Mapping) or hasattr(item, "keys"):
        try:
            return DuplicateFile.from_row(item)
        except ValueError:
            return DuplicateFile(file_id=-1, path=Path(""), size=None, width=None, height=None, phash=None)
    return DuplicateFile(file_id=-1, path=Path(""), size=None, width=None, height=None,              # a PIL image
                         phash=compute_signature(item, device=device)[0] & ((1 << 64) - 1))


def find_similar(library: Iterable, queries: Iterable, *, k: int = 10, max_distance: Optional[int] = None, device: Optional[int] = None,
                 scanner_factory: Callable[[DuplicateScanConfig], DuplicateScanner] = DuplicateScanner) -> list:
    """For every query the ``k`` library files most like it, best first: one list of ``SimilarFile(file, distance)`` per
    query, ordered by the Hamming distance of the pHashes, ties by the file's place in ``library``
    (``DuplicateScanner.nearest``).  A ranked, threshold-free answer: no band predicate, no size filter -- it finds the
    pairs 4..8 bits apart that share no 16-bit band, which ``find_duplicates`` links only with ``exact=True``.

    ``library``: as ``files`` of ``find_duplicates``.  An item of ``queries`` is a DuplicateFile, a row mapping, or a ``str`` /
    ``Path`` / PIL image; the last three are hashed here through ``compute_signature``, one at a time -- meant for a handful of
    queries, hash a collection with the batch hasher instead -- and carry no file id.  A query with a file id never gets the
    library file of that id; a query without a usable hash gets [].  ``max_distance``: leave out files further away (None:
    64, no limit).  ``k`` is at most 1024."""
    device = 0 if device is None else int(device)
    files = _parse_files(library)
    asked = [_parse_query(item, device) for item in queries]
    scanner = _make_scanner(scanner_factory, DuplicateScanConfig(), device)
    return scanner.nearest(files, asked, k, max_distance)


def _turned_matches(scanner, candidates, turned, ok) -> list:
    return scanner.turned_edges(candidates, turned, ok)


def _trimmed_matches(scanner, candidates, hashes, boxes, has, ok) -> list:
    return scanner.trimmed_edges(candidates, hashes, has & ok, boxes)


def _turned_trimmed_matches(scanner, candidates, turned, cut, boxes, has, ok) -> list:
    """The best match per pair of files, by ``view_rank``, over ``trimmed_edges`` on the crops as they lie (orientation 0) and
    ``turned_trimmed_edges`` (orientations 1..7)."""
    from .scanner import TransformedMatch, view_rank

    found = [TransformedMatch(m.file_id_a, m.file_id_b, m.trimmed_a, m.trimmed_b, 0, m.hamming, m.box_a, m.box_b)
             for m in scanner.trimmed_edges(candidates, cut[:, 0], has & ok, boxes)]
    found += scanner.turned_trimmed_edges(candidates, turned, cut, has & ok, ok, boxes)
    best: dict = {}
    for m in found:
        key = (m.file_id_a, m.file_id_b)
        rank = view_rank(m.hamming, m.orientation, m.trimmed_a, m.trimmed_b)
        if key not in best or rank < best[key][0]:
            best[key] = (rank, m)
    return [best[key][1] for key in sorted(best)]


# The view searches, by mode: (the module and the function that make the signatures -- looked up when called --, whether
# ``tolerance`` applies, what turns (scanner, candidates, *signatures) into matches, the refine call of the SSIM re-check, the
# attributes of a match that follow the ids and paths in a row of that call).  A further view is a row here.
_VIEW_MODES = {
    "turned": ("turned", "turned_signatures", False, _turned_matches, "refine_turned_pairs", ("orientation",)),
    "trimmed": ("trimmed", "trimmed_signatures", True, _trimmed_matches, "refine_trimmed_pairs", ("trimmed_a", "trimmed_b")),
    "turned_trimmed": ("turned_trimmed", "turned_trimmed_signatures", True, _turned_trimmed_matches, "refine_turned_trimmed_pairs",
                       ("trimmed_a", "trimmed_b", "orientation")),
}


def _view_scan(mode: str, files: Iterable, *, hamming_threshold, size_ratio, band_bits, band_count, device, tolerance=None,
               ssim_threshold=None, exact=False) -> tuple:
    """The work of find_turned_duplicates, find_trimmed_duplicates and find_turned_trimmed_duplicates (``mode``: a key of
    _VIEW_MODES): (clusters, matches, the (id, id) keys of the plain candidate edges).  With ``ssim_threshold`` the matches and
    the keys are the ones that passed the re-check.  ``tolerance`` is read by the modes that trim.  ``exact``: the plain scan and
    the view scan both take every pair within the threshold (``DuplicateScanConfig.exact``)."""
    from .scanner import DuplicateEdge, assemble_clusters

    module, signatures, takes_tolerance, collect, refine_name, tail = _VIEW_MODES[mode]
    candidates = [f for f in _parse_files(files) if f.phash is not None]
    if len(candidates) < 2:
        return [], [], set()
    keywords = {"tolerance": tolerance} if takes_tolerance else {}
    config = DuplicateScanConfig(hamming_threshold=hamming_threshold, size_ratio=size_ratio, band_bits=band_bits,
                                 band_count=band_count, exact=bool(exact))
    scanner = DuplicateScanner(config, device=device)
    made = getattr(importlib.import_module("." + module, __package__), signatures)([f.path for f in candidates], device=device, **keywords)
    plain = scanner.candidate_edges(candidates)
    matches = collect(scanner, candidates, *made)
    if ssim_threshold is not None and (plain or matches):
        plain, matches = _views_ssim_kept(refine_name, tail, plain, matches, candidates, ssim_threshold, device, **keywords)
    edges = list(plain.values()) + [DuplicateEdge(m.file_id_a, m.file_id_b, m.hamming) for m in matches]
    return (assemble_clusters(candidates, edges) if edges else []), matches, set(plain)


def _views_ssim_kept(refine_name: str, tail: tuple, plain: dict, matches: list, candidates: Sequence[DuplicateFile], ssim_threshold: float,
                     device: int, **keywords) -> tuple:
    """The plain candidate edges and the matches that pass the SSIM re-check, from one call of ``refine.<refine_name>``: a row
    is the two ids and paths and then the match's ``tail`` attributes; a plain edge is scored as the pixels lie (every flag
    False, orientation 0).  A surviving match carries its score; a pair whose files cannot be read is dropped, as _ssim_kept
    drops it."""
    from dataclasses import replace

    by_id = {f.file_id: f for f in candidates}
    keys = list(plain)
    as_it_lies = tuple(0 if name == "orientation" else False for name in tail)
    rows = [(plain[k].file_id_a, plain[k].file_id_b, by_id[plain[k].file_id_a].path, by_id[plain[k].file_id_b].path) + as_it_lies for k in keys]
    rows += [(m.file_id_a, m.file_id_b, by_id[m.file_id_a].path, by_id[m.file_id_b].path) + tuple(getattr(m, name) for name in tail)
             for m in matches]
    refined = getattr(_refine, refine_name)(rows, thresholds=_refine.RefinementThresholds(ssim=ssim_threshold), device=device, **keywords)
    passed = [r is not None and r.is_duplicate for r in refined]
    kept_plain = {k: plain[k] for k, yes in zip(keys, passed) if yes}
    kept_matches = [replace(m, ssim=r.ssim) for m, r, yes in zip(matches, refined[len(keys):], passed[len(keys):]) if yes]
    return kept_plain, kept_matches


def find_turned_duplicates(files: Iterable, *, hamming_threshold: int = 8, size_ratio: Optional[float] = None, band_bits: int = 16,
                           band_count: int = 4, device: Optional[int] = None, ssim_threshold: Optional[float] = None,
                           exact: bool = False) -> tuple:
    """(clusters, matches): near-duplicates including mirrored, flipped and rotated copies.

    ``files``: as for ``find_duplicates``, each with a readable ``path``: the files are read and the pHashes of their
    eight orientations made from the 32x32 tile the hash kernels form (``turned.turned_signatures``; nothing is stored).
    ``matches``: the ``scanner.TurnedMatch`` list of ``DuplicateScanner.turned_edges`` -- file a, file b, the orientation
    that turns b's picture into a's, the hamming distance.  ``clusters``: ``assemble_clusters`` over the plain candidate
    edges of the stored hashes together with the matches as edges.  A file whose turned hashes could not be made (Pillow
    cannot open it) takes part with its stored pHash only.

    With ``ssim_threshold`` set, every plain candidate edge and every match is re-checked on the files' pixels, a match as
    file a against its orientation of file b, turned on the device (``refine.refine_turned_pairs``, one call for all).
    Only edges with ``ssim >= ssim_threshold`` reach the clusters, and ``matches`` holds the surviving matches, each with
    its ``ssim``.  A pair that is both a plain edge and a match stays linked if either passes; a pair with an unreadable
    file is dropped.  Unset: no pixels are compared and ``ssim`` is None.  ``exact``: as for ``find_duplicates``, for the plain
    edges and the matches alike -- a turned copy 6 bits away with a flipped bit in every band is then a match.

    Out of scope here: persisting turned hashes, ``devices=[...]`` (one process, one GPU) and dHash.  A copy that is turned AND has a
    margin round it is ``find_turned_trimmed_duplicates``'."""
    return _view_scan("turned", files, hamming_threshold=hamming_threshold, size_ratio=size_ratio, band_bits=band_bits,
                      band_count=band_count, device=0 if device is None else int(device), ssim_threshold=ssim_threshold, exact=exact)[:2]


def find_trimmed_duplicates(files: Iterable, *, hamming_threshold: int = 8, tolerance: int = 48, size_ratio: Optional[float] = None,
                            band_bits: int = 16, band_count: int = 4, device: Optional[int] = None,
                            ssim_threshold: Optional[float] = None, exact: bool = False) -> tuple:
    """(clusters, matches): near-duplicates including copies with a margin round them -- letterboxed, pillarboxed, framed,
    on a white page, on a larger canvas.

    ``files``: as for ``find_duplicates``, each with a readable ``path``: the files are read, their content boxes found on
    the device (include/keyes.h, ``ke_content_boxes``: the pixels farther than ``tolerance`` from the corner pixel) and the
    pHash of every qualifying box made (``trimmed.trimmed_signatures``; nothing is stored).  ``matches``: the
    ``scanner.TrimmedMatch`` list of ``DuplicateScanner.trimmed_edges`` -- file a, file b, which side was cut, the hamming
    distance, the boxes.  ``clusters``: ``assemble_clusters`` over the plain candidate edges of the stored hashes together
    with the matches as edges.  A file without a qualifying box, or one that cannot be opened, takes part with its stored
    pHash only.

    With ``ssim_threshold`` set, every plain candidate edge and every match is re-checked on the files' pixels, a match with
    each trimmed side cut to its content box on the device -- the box of the pixels as the refine seam decodes them, found
    there (``refine.refine_trimmed_pairs``, one call for all).  Only edges with ``ssim >= ssim_threshold`` reach the clusters,
    and ``matches`` holds the surviving matches, each with its ``ssim``.  A pair that is both a plain edge and a match stays
    linked if either passes; a pair with an unreadable file is dropped.  Unset: no pixels are compared and ``ssim`` is None.
    ``exact``: as for ``find_duplicates``, for the plain edges and the matches alike.

    Out of scope here: an MAE re-check on the crop, ``devices=[...]`` (one process, one GPU), persisting trimmed
    hashes, borders of two colours or gradients, and dHash.  Trimmed and turned together is ``find_turned_trimmed_duplicates``'."""
    return _view_scan("trimmed", files, hamming_threshold=hamming_threshold, tolerance=tolerance, size_ratio=size_ratio, band_bits=band_bits,
                      band_count=band_count, device=0 if device is None else int(device), ssim_threshold=ssim_threshold, exact=exact)[:2]


def find_turned_trimmed_duplicates(files: Iterable, *, hamming_threshold: int = 8, tolerance: int = 48, size_ratio: Optional[float] = None,
                                   band_bits: int = 16, band_count: int = 4, device: Optional[int] = None,
                                   ssim_threshold: Optional[float] = None, exact: bool = False) -> tuple:
    """(clusters, matches): near-duplicates including copies that were given a margin, turned, or both -- a scan laid on the
    glass sideways with a white margin, a letterboxed frame that was mirrored, a framed repost rotated a quarter turn.

    ``files``: as for ``find_duplicates``, each with a readable ``path``.  Every file is read once
    (``turned_trimmed.turned_trimmed_signatures``; nothing is stored): the eight turned pHashes of the picture, its content box
    at ``tolerance``, and the eight turned pHashes of the picture cut to a qualifying box.  ``matches``: ``scanner.TransformedMatch``
    -- file a, file b, which side was cut, the orientation that turns b's (cut) picture into a's (cut) picture, the hamming
    distance, the boxes --, the best per pair of files, by (hamming, orientation, trimmed_a, trimmed_b), over
    ``DuplicateScanner.trimmed_edges`` (orientation 0) and ``DuplicateScanner.turned_trimmed_edges`` (orientations 1..7, either
    side whole or cut).  Plain edges stay edges.  ``clusters``: ``assemble_clusters`` over the plain candidate edges of the
    stored hashes together with the matches as edges.  A file that cannot be opened takes part with its stored pHash only.

    With ``ssim_threshold`` set, every plain candidate edge and every match is re-checked on the files' pixels by one
    ``refine.refine_turned_trimmed_pairs`` call: a's view against b's, cut (to the box found at that seam) and turned on the
    device.  Only edges with ``ssim >= ssim_threshold`` reach the clusters, and ``matches`` holds the surviving matches, each
    with its ``ssim``.  A pair that is both a plain edge and a match stays linked if either passes; a pair with an unreadable
    file is dropped.  Unset: no pixels are compared and ``ssim`` is None.  ``exact``: as for ``find_duplicates``, for the plain
    edges and the matches alike.

    Out of scope here: ``devices=[...]`` (one process, one GPU), persisting any of these hashes, turning side a, dHash, borders
    of two colours or gradients, and an MAE re-check."""
    return _view_scan("turned_trimmed", files, hamming_threshold=hamming_threshold, tolerance=tolerance, size_ratio=size_ratio,
                      band_bits=band_bits, band_count=band_count, device=0 if device is None else int(device),
                      ssim_threshold=ssim_threshold, exact=exact)[:2]


def run_duplicate_scan(rows: Sequence[Mapping], *, db_path: Optional[str] = None, config: Optional[DuplicateScanConfig] = None,
                       progress: Optional[Callable[[str, int, int], None]] = None,
                       cancel_fn: Optional[Callable[[], bool]] = None, device: Optional[int] = None,
                       devices: Optional[Sequence[int]] = None) -> list:
    """Headless ``DuplicateScanRunnable.run``: stage names and order as the reference emits them.  ``devices``: the missing
    signatures are computed by one worker process per entry (``fast_fill_missing_signatures``); the scan and the clusters stay
    in this process, on ``device`` (default ``devices[0]``, else 0).  An exact scan is asked for through ``config``
    (``DuplicateScanConfig(exact=True)``)."""
    if device is None:
        device = int(devices[0]) if devices else 0
    def tick(stage, done, total):
        if progress:
            progress(stage, done, total)

    rows = [dict(r) for r in rows]
    tick("Loading files", len(rows), len(rows))
    missing = [(int(r.get("file_id", r.get("id"))), str(r["path"])) for r in rows
               if r.get("phash_u64") is None and r.get("path")]
    if missing:
        filled = fastsig.fast_fill_missing_signatures(
            db_path or ":memory:", missing, max_workers=8, chunksize=64, apply_to_db=db_path is not None,
            progress=lambda d, t: tick("Computing signatures", d, t), cancel_fn=cancel_fn, device=device,
            devices=devices)
        by_id = {fid: ph for fid, ph, _ in filled}
        for r in rows:
            fid = int(r.get("file_id", r.get("id")))
            if r.get("phash_u64") is None and fid in by_id:
                r["phash_u64"] = by_id[fid]
    if cancel_fn and cancel_fn():
        return []
    tick("Building groups", 0, len(rows))
    files = []
    for r in rows:
        try:
            files.append(DuplicateFile.from_row(r))
        except ValueError:
            continue
    tick("Clustering duplicates", 0, len(files))
    return DuplicateScanner(config or DuplicateScanConfig(), device=device).build_clusters(files)


__all__ = ["DedupSettings", "compute_signature", "find_duplicates", "find_similar", "SimilarFile", "find_new_duplicates", "find_turned_duplicates", "find_trimmed_duplicates",
           "find_turned_trimmed_duplicates", "run_duplicate_scan", "ClusterBuilder"]
