"""Headless duplicate scan over a kobato-eyes SQLite database.

    python -m kobato_eyes_amd.cli scan-dups --db kobato.db --hamming 8 [--like '%/photos/%'] [--size-ratio 0.5]
                                            [--added-like '%/incoming/%'] [--refine] [--csv out.csv] [--device 0]
                                            [--devices 0,1,2] [--turned [--turned-ssim 0.9]]
                                            [--trimmed [--trim-tolerance 48] [--trimmed-ssim 0.9]]
                                            [--turned-trimmed [--trim-tolerance 48] [--turned-trimmed-ssim 0.9]]
                                            [--exact]
    python -m kobato_eyes_amd.cli similar --db kobato.db (--to PATH ... | --to-like '%/incoming/%') [--like '%/photos/%']
                                          [--k 10] [--max-distance N] [--csv out.csv] [--device 0]

Reproduces the call sequence of DuplicateScanRunnable.run (src/ui/dup_workers.py:148-239) without Qt: rows in
the shape of db.repository.iter_files_for_dup (src/db/repository.py:416-454), missing signatures filled and
upserted as core.fastsig does (src/core/fastsig.py:102-126), DuplicateFile.from_row with bad rows skipped,
build_clusters, optionally the shipped refine pipeline (tile aHash max_bits, then pixel MAE 0.004 as
src/ui/dup_tab.py:302-311 wires it), and the CSV layout of export_duplicate_clusters_csv
(src/ui/file_actions.py:61-80).
"""
from __future__ import annotations

import argparse
import csv
import logging
import os
import sqlite3
import sys
from typing import Iterator, Optional, Sequence

CSV_HEADER = ["group", "file_id", "path", "size", "width", "height", "keeper", "hamming"]


def iter_files_for_dup(conn: sqlite3.Connection, path_like: Optional[str], added_like: Optional[str] = None) -> Iterator[dict]:
    """Plain dicts with file_id, path, size, width, height, phash_u64 for every present file, by id.  With ``added_like``
    each dict also says under "added" whether the path matches that LIKE pattern."""
    sql = ("SELECT f.id AS file_id, f.path AS path, COALESCE(f.size, 0) AS size, f.width AS width, f.height AS height, "
           "s.phash_u64 AS phash_u64")
    params: list = []
    if added_like:
        sql += ", f.path LIKE ? ESCAPE '\\' AS added"
        params.append(added_like)
    sql += " FROM files f LEFT JOIN signatures s ON s.file_id = f.id WHERE f.is_present = 1"
    if path_like:
        sql += " AND f.path LIKE ? ESCAPE '\\'"
        params.append(path_like)
    sql += " ORDER BY f.id"
    for row in conn.execute(sql, params):
        item = {"file_id": row[0], "path": row[1], "size": row[2], "width": row[3], "height": row[4], "phash_u64": row[5]}
        if added_like:
            item["added"] = bool(row[6])
        yield item


def export_duplicate_clusters_csv(clusters: Sequence, file_path, orientations: Optional[dict] = None, boxes: Optional[dict] = None) -> None:
    """``orientations`` (scan-dups --turned): {file_id: orientation}; the CSV then has a ninth column ``orientation``,
    filled for the files that are linked to their group's keeper only through a turn (``orientations_to_keeper``).
    ``boxes`` (scan-dups --trimmed): {file_id: (x0, y0, x1, y1)}; the ninth column is then ``box``, ``x0 y0 x1 y1`` for a file
    that is linked through its content box (``boxes_of_matches``) and empty for a file linked as it is.  With both (scan-dups
    --turned-trimmed) ``orientation`` is the ninth column and ``box`` the tenth."""
    with open(file_path, "w", encoding="utf-8", newline="") as handle:
        writer = csv.writer(handle)
        writer.writerow(CSV_HEADER + (["orientation"] if orientations is not None else []) + (["box"] if boxes is not None else []))
        for group, cluster in enumerate(clusters, start=1):
            for entry in cluster.files:
                f = entry.file
                row = [group, f.file_id, f.path.as_posix(), f.size or 0, f.width or 0, f.height or 0,
                       1 if f.file_id == cluster.keeper_id else 0,
                       entry.best_hamming if entry.best_hamming is not None else ""]
                if orientations is not None:
                    row.append(orientations.get(f.file_id, ""))
                if boxes is not None:
                    row.append(" ".join(str(v) for v in boxes[f.file_id]) if f.file_id in boxes else "")
                writer.writerow(row)


def boxes_of_matches(matches: Sequence) -> dict:
    """{file_id: box} for the files that some ``scanner.TrimmedMatch`` or ``scanner.TransformedMatch`` links through their
    content box."""
    out: dict = {}
    for m in matches:
        if m.trimmed_a and m.box_a is not None:
            out[m.file_id_a] = m.box_a
        if m.trimmed_b and m.box_b is not None:
            out[m.file_id_b] = m.box_b
    return out


def orientations_to_keeper(clusters: Sequence, matches: Sequence, plain_keys) -> dict:
    """{file_id: orientation} for the files that are linked to their group's keeper only through a turn: the orientation
    (turned.ORIENTATIONS) that brings the file's picture to the keeper's.  Worked out group by group from the keeper
    outwards: a plain candidate edge (``plain_keys``: their (id, id) keys) carries the identity, a turned match its
    orientation or the inverse, plain edges first; files that come out with the identity are left out."""
    from .turned import COMPOSE, INVERSE

    links: dict = {}
    for a, b in plain_keys:
        links.setdefault(a, []).append((b, 0))
        links.setdefault(b, []).append((a, 0))
    for m in matches:                                   # orientation turns b's picture into a's
        links.setdefault(m.file_id_a, []).append((m.file_id_b, m.orientation))
        links.setdefault(m.file_id_b, []).append((m.file_id_a, INVERSE[m.orientation]))
    out: dict = {}
    for cluster in clusters:
        to_keeper = {cluster.keeper_id: 0}
        queue = [cluster.keeper_id]
        while queue:
            f = queue.pop(0)
            for g, t in sorted(links.get(f, ()), key=lambda link: (link[1] != 0, link[0])):   # t turns g's picture into f's
                if g not in to_keeper:
                    to_keeper[g] = COMPOSE[t][to_keeper[f]]
                    queue.append(g)
        out.update({f: k for f, k in to_keeper.items() if k})
    return out


def load_files_for_dup(db_path: str, path_like: Optional[str], added_like: Optional[str] = None, *, device: int = 0,
                       devices: Optional[Sequence[int]] = None, tick=lambda stage, done, total: None) -> tuple:
    """(rows, files) of a selection: the rows of ``iter_files_for_dup`` with missing signatures computed and upserted as
    core.fastsig does, and their DuplicateFile objects, rows still without a hash skipped as the reference does."""
    from . import DuplicateFile, fast_fill_missing_signatures

    conn = sqlite3.connect(db_path)
    try:
        rows = list(iter_files_for_dup(conn, path_like, added_like))
    finally:
        conn.close()
    tick("Loading files", len(rows), len(rows))
    missing = [(r["file_id"], r["path"]) for r in rows if r["phash_u64"] is None and r["path"]]
    if missing:
        workers = int(os.environ.get("KE_SIG_WORKERS", "8"))
        chunk = int(os.environ.get("KE_SIG_CHUNK", "64"))
        filled = fast_fill_missing_signatures(db_path, missing, max_workers=workers, chunksize=chunk,
                                              progress=lambda d, t: tick("Computing signatures", d, t), device=device,
                                              devices=devices)
        by_id = {fid: ph for fid, ph, _ in filled}
        for r in rows:
            if r["phash_u64"] is None:
                r["phash_u64"] = by_id.get(r["file_id"])
    tick("Building groups", 0, len(rows))
    files = []
    for r in rows:
        try:
            files.append(DuplicateFile.from_row(r))
        except ValueError:
            continue                                   # rows still without a hash are skipped, as the reference does
    return rows, files


SIMILAR_HEADER = ["query", "rank", "path", "distance"]


def similar_in_database(db_path: str, *, to: Sequence[str] = (), to_like: Optional[str] = None, path_like: Optional[str] = None,
                        k: int = 10, max_distance: Optional[int] = None, device: Optional[int] = None) -> list:
    """[(query, rank, path, distance)], rank from 1, for the ``similar`` sub-command: the library is the selection
    (``path_like``) loaded as scan-dups loads it; the queries are either the files of the selection whose path matches
    ``to_like`` -- each left out of its own answer -- or the files ``to``, which are hashed here and need not be in the
    database.  Ranking by pHash distance alone (``find_similar``): no threshold, no band predicate."""
    from .api import find_similar

    if bool(to) == bool(to_like):
        raise ValueError("similar needs either --to PATH ... or --to-like PATTERN")
    device = 0 if device is None else int(device)
    rows, files = load_files_for_dup(db_path, path_like, to_like, device=device)
    if to_like:
        asked_ids = {r["file_id"] for r in rows if r["added"]}
        queries = [f for f in files if f.file_id in asked_ids]
        names = [f.path.as_posix() for f in queries]
    else:
        queries, names = list(to), [str(p) for p in to]
    found = find_similar(files, queries, k=k, max_distance=max_distance, device=device)
    return [(name, rank, hit.file.path.as_posix(), hit.distance)
            for name, hits in zip(names, found) for rank, hit in enumerate(hits, start=1)]


# what a view search of scan_database hands out besides the clusters: mode -> (orientations_out is filled, boxes_out is filled)
VIEW_COLUMNS = {"turned": (True, False), "trimmed": (False, True), "turned_trimmed": (True, True)}


def scan_database(db_path: str, *, hamming_threshold: int = 8, size_ratio: Optional[float] = None, path_like: Optional[str] = None,
                  refine: bool = False, tile_max_bits: int = 32, mae_thr: float = 0.004, device: Optional[int] = None, progress=None,
                  devices: Optional[Sequence[int]] = None, added_like: Optional[str] = None, turned: bool = False,
                  orientations_out: Optional[dict] = None, turned_ssim: Optional[float] = None, trimmed: bool = False,
                  trim_tolerance: int = 48, boxes_out: Optional[dict] = None, trimmed_ssim: Optional[float] = None,
                  turned_trimmed: bool = False, turned_trimmed_ssim: Optional[float] = None, exact: bool = False) -> list:
    """``devices``: the missing signatures are computed by one worker process per entry; the scan and the tile-aHash / MAE
    refine stay in this process, on ``device`` (default ``devices[0]``, else 0).  ``added_like``: the files of the
    selection whose path matches this LIKE pattern are the added set, the rest the library; only the pairs that touch an
    added file are scanned and only the clusters with an added member come back (``find_new_duplicates`` without
    ``previous``: a link between two library files is absent).  ``turned``: the files of the selection are read and
    mirrored, flipped and rotated copies are linked as well (``find_turned_duplicates``; not together with
    ``added_like`` or ``refine``); ``orientations_out`` then receives ``orientations_to_keeper`` of the result.
    ``turned_ssim`` (only with ``turned``): the candidate edges and the turned matches are re-checked with SSIM, a match with
    one file turned on the device, and only those at or above this score link files (``find_turned_duplicates``'
    ``ssim_threshold``); the orientations are then worked out from the survivors.  ``trimmed``: the files of the selection
    are read and copies with a margin round them are linked as well (``find_trimmed_duplicates`` with ``trim_tolerance``;
    not together with ``turned``, ``added_like`` or ``refine``); ``boxes_out`` then receives ``boxes_of_matches`` of the
    result.  ``trimmed_ssim`` (only with ``trimmed``): the candidate edges and the trimmed matches are re-checked with SSIM, a
    match with its trimmed sides cut to their content boxes on the device, and only those at or above this score link files
    (``find_trimmed_duplicates``' ``ssim_threshold``); the boxes are then those of the survivors.  ``turned_trimmed``: a mode of
    its own -- copies that were given a margin, turned, or both are linked (``find_turned_trimmed_duplicates`` with
    ``trim_tolerance``; not together with ``turned``, ``trimmed``, ``added_like`` or ``refine``); ``orientations_out`` and
    ``boxes_out`` receive what they receive in those two modes.  ``turned_trimmed_ssim`` (only with ``turned_trimmed``): its
    ``ssim_threshold``.  ``exact``: in whichever mode, every pair within ``hamming_threshold`` links, whether or not it shares a
    16-bit band (``DuplicateScanConfig.exact``)."""
    if turned_trimmed_ssim is not None and not turned_trimmed:
        raise ValueError("--turned-trimmed-ssim needs --turned-trimmed")
    if turned_trimmed and (turned or trimmed or added_like or refine):
        # --turned and --trimmed are this mode's halves; the refine pipeline compares whole pictures as they lie
        raise ValueError("--turned-trimmed cannot be combined with --turned, --trimmed, --added-like or --refine")
    if turned_ssim is not None and not turned:
        raise ValueError("--turned-ssim needs --turned")
    if trimmed_ssim is not None and not trimmed:
        raise ValueError("--trimmed-ssim needs --trimmed")
    if trimmed and (turned or added_like or refine):
        # the refine pipeline compares whole pictures and would cut every link that exists through a crop
        raise ValueError("--trimmed cannot be combined with --turned, --added-like or --refine")
    if turned and (added_like or refine):
        # the refine pipeline compares pixels as they lie and would cut every link that exists through a turn
        raise ValueError("--turned cannot be combined with --added-like or --refine")
    from . import DuplicateScanConfig, DuplicateScanner
    from .refine_parallel import refine_by_pixels_parallel, refine_by_tilehash_parallel

    if device is None:
        device = int(devices[0]) if devices else 0

    def tick(stage, done, total):
        if progress:
            progress(stage, done, total)

    rows, files = load_files_for_dup(db_path, path_like, added_like, device=device, devices=devices, tick=tick)
    tick("Clustering duplicates", 0, len(files))
    mode, ssim_threshold = (("turned_trimmed", turned_trimmed_ssim) if turned_trimmed else ("turned", turned_ssim) if turned else
                            ("trimmed", trimmed_ssim) if trimmed else (None, None))
    if mode:
        from .api import _view_scan

        orientations, boxes = VIEW_COLUMNS[mode]
        clusters, matches, plain_keys = _view_scan(mode, files, hamming_threshold=hamming_threshold, tolerance=trim_tolerance,
                                                   size_ratio=size_ratio, band_bits=16, band_count=4, device=device,
                                                   ssim_threshold=ssim_threshold, exact=exact)
        if orientations and orientations_out is not None:
            orientations_out.update(orientations_to_keeper(clusters, matches, plain_keys))
        if boxes and boxes_out is not None:
            boxes_out.update(boxes_of_matches(matches))
    elif added_like:
        from .api import find_new_duplicates

        added_ids = {r["file_id"] for r in rows if r["added"]}
        clusters = find_new_duplicates([f for f in files if f.file_id not in added_ids], [f for f in files if f.file_id in added_ids],
                                       hamming_threshold=hamming_threshold, size_ratio=size_ratio, device=device, exact=exact)
    else:
        clusters = DuplicateScanner(DuplicateScanConfig(hamming_threshold=hamming_threshold, size_ratio=size_ratio, exact=bool(exact)),
                                    device=device).build_clusters(files)
    if refine and clusters:
        clusters = refine_by_tilehash_parallel(clusters, max_bits=tile_max_bits, device=device,
                                               tick=lambda d, t, phase: tick(f"Refining (tile hash {phase}/2)", d, t))
        clusters = refine_by_pixels_parallel(clusters, mae_thr=mae_thr, device=device,
                                             tick=lambda d, t: tick("Refining (pixels)", d, t))
    return clusters


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="kobato_eyes_amd.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    sp = sub.add_parser("scan-dups", help="cluster near-duplicate files of a kobato-eyes database")
    sp.add_argument("--db", required=True)
    sp.add_argument("--hamming", type=int, default=8)
    sp.add_argument("--size-ratio", type=float, default=None)
    sp.add_argument("--like", default=None, help="SQL LIKE pattern on files.path")
    sp.add_argument("--added-like", default=None,
                    help="SQL LIKE pattern: the matching files of the selection are newly added, the rest is the library; only "
                         "pairs with an added file are scanned and only groups with an added file are reported")
    sp.add_argument("--turned", action="store_true",
                    help="read the files of the selection and link mirrored, flipped and rotated copies as well; the CSV gains an "
                         "orientation column: the turn that brings a file's picture to its group's keeper's")
    sp.add_argument("--turned-ssim", type=float, default=None,
                    help="with --turned: re-check every candidate edge and turned match with SSIM on the pixels (one file turned on "
                         "the device for a match) and link only those at or above this score, e.g. 0.9")
    sp.add_argument("--trimmed", action="store_true",
                    help="read the files of the selection and link copies with a margin round them as well (letterbox, pillarbox, "
                         "frame, white page); the CSV gains a box column: x0 y0 x1 y1 of a file linked through its content box")
    sp.add_argument("--trim-tolerance", type=int, default=48,
                    help="with --trimmed: a pixel belongs to the content when a channel lies farther than this from the corner pixel")
    sp.add_argument("--trimmed-ssim", type=float, default=None,
                    help="with --trimmed: re-check every candidate edge and trimmed match with SSIM on the pixels (a trimmed side cut "
                         "to its content box on the device) and link only those at or above this score, e.g. 0.9")
    sp.add_argument("--turned-trimmed", action="store_true",
                    help="a mode of its own: read the files of the selection and link copies that were given a margin, turned, or both; "
                         "the CSV gains an orientation and a box column; --trim-tolerance applies")
    sp.add_argument("--turned-trimmed-ssim", type=float, default=None,
                    help="with --turned-trimmed: re-check every candidate edge and match with SSIM on the pixels (cut and turned on the "
                         "device) and link only those at or above this score, e.g. 0.9")
    sp.add_argument("--exact", action="store_true",
                    help="link every pair within --hamming bits, whether or not it shares a 16-bit band (without it a pair links "
                         "only when one of the four bands is equal, so --hamming above about 8 finds nothing more); combines with "
                         "every mode above")
    sp.add_argument("--refine", action="store_true", help="run the tile-aHash + pixel-MAE refine pipeline on the clusters")
    sp.add_argument("--tile-max-bits", type=int, default=32)
    sp.add_argument("--mae-thr", type=float, default=0.004)
    sp.add_argument("--csv", default=None)
    sp.add_argument("--device", type=int, default=None, help="where the scan and the refine run (default: the first of --devices, else 0)")
    sp.add_argument("--devices", default=None, type=lambda text: [int(d) for d in text.split(",") if d.strip()],
                    help="e.g. 0,1,2: missing signatures are computed by one worker process per entry (at most 15)")
    sp.add_argument("-v", "--verbose", action="store_true")
    sm = sub.add_parser("similar", help="rank the files of a kobato-eyes database by pHash distance to given pictures")
    sm.add_argument("--db", required=True)
    target = sm.add_mutually_exclusive_group(required=True)
    target.add_argument("--to", nargs="+", default=None, metavar="PATH", help="picture files to find neighbours of; they need not be in the database")
    target.add_argument("--to-like", default=None,
                        help="SQL LIKE pattern: the matching files of the selection are the queries, each left out of its own answer")
    sm.add_argument("--like", default=None, help="SQL LIKE pattern on files.path: the library")
    sm.add_argument("--k", type=int, default=10, help="neighbours per query, at most 1024")
    sm.add_argument("--max-distance", type=int, default=None, help="leave out files more than this many bits away (default: no limit)")
    sm.add_argument("--csv", default=None)
    sm.add_argument("--device", type=int, default=None)
    sm.add_argument("-v", "--verbose", action="store_true")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARNING)
    if args.cmd == "similar":
        found = similar_in_database(args.db, to=args.to or (), to_like=args.to_like, path_like=args.like, k=args.k,
                                    max_distance=args.max_distance, device=args.device)
        handle = open(args.csv, "w", encoding="utf-8", newline="") if args.csv else sys.stdout
        try:
            writer = csv.writer(handle)
            writer.writerow(SIMILAR_HEADER)
            writer.writerows(found)
        finally:
            if args.csv:
                handle.close()
        if args.csv:
            print(f"{len(found)} neighbour(s) of {len({row[0] for row in found})} querie(s) -> {args.csv}")
        return 0
    orientations = {} if args.turned or args.turned_trimmed else None
    boxes = {} if args.trimmed or args.turned_trimmed else None
    clusters = scan_database(args.db, hamming_threshold=args.hamming, size_ratio=args.size_ratio, path_like=args.like,
                             refine=args.refine, tile_max_bits=args.tile_max_bits, mae_thr=args.mae_thr, device=args.device,
                             devices=args.devices, added_like=args.added_like, turned=args.turned, orientations_out=orientations,
                             turned_ssim=args.turned_ssim, trimmed=args.trimmed, trim_tolerance=args.trim_tolerance, boxes_out=boxes,
                             trimmed_ssim=args.trimmed_ssim, turned_trimmed=args.turned_trimmed,
                             turned_trimmed_ssim=args.turned_trimmed_ssim, exact=args.exact)
    if args.csv:
        export_duplicate_clusters_csv(clusters, args.csv, orientations, boxes)
    members = sum(len(c.files) for c in clusters)
    print(f"{len(clusters)} duplicate group(s), {members} file(s)" + (f" -> {args.csv}" if args.csv else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
