"""Turned pHashes (ke_tiles_turned, ke_hash_images_turned: ke_tiles_to_phash_turned of csrc/ke_hash.hip), the cross scan
(ke_hamming_scan_cross: ke_scan_tiles_cross and ke_bucket_pairs_cross of csrc/ke_scan.hip) and what is built on them.

The hashes are held to the CPU oracle bit for bit: column k is O.phash_from_tile of orientation k of the oracle's tile.  That
the tile's turned hash stands for the really turned image's is tests/test_turned_cpu.py's business (at most 2 bits, 0 for the
flips, on these very images).  The cross scan runs on the tables of tests/_scan_from_cases.py under KE_SCAN_MODE=auto, tiles
and buckets, each mode in a fresh child process (the library reads the mode once), one after the other: the sorted
(a, b, h, bands) equal the oracle's banded scan filtered by a < first_new <= b and the full ke_hamming_scan filtered the same
way."""
from __future__ import annotations

import csv
import os
import sqlite3
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _scan_from_cases as S
import _turned_cases as T
import kobato_eyes_amd as K
from kobato_eyes_amd import _native, api, cli, turned
from kobato_eyes_amd.scanner import DuplicateFile, TurnedMatch
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("auto", "tiles", "buckets")
CASES = S.small_cases()


@pytest.fixture(scope="module")
def ctx():
    return _native.get_context(0)


def _oracle_turned(tile) -> list:
    return [O.phash_from_tile(T.turn_k(k, tile))[0] for k in range(8)]


# ---- tiles --------------------------------------------------------------------------------------------------------------
def test_tiles_turned_equals_the_oracle_on_every_turned_tile(ctx):
    names, tiles = T.tiles()
    assert len(tiles) >= 40
    # one call: the tiles themselves, then orientation j of every tile for j = 1..7
    batch = np.concatenate([tiles] + [np.stack([T.turn_k(j, t) for t in tiles]) for j in range(1, 8)])
    got = ctx.tiles_turned(batch)
    assert got.shape == (8 * len(tiles), 8) and got.dtype == np.uint64
    own = got[: len(tiles)]
    for i, name in enumerate(names):
        assert own[i].tolist() == _oracle_turned(tiles[i]), name
    assert own[names.index("flat0")].tolist() == [0] * 8                       # 0 > 0 is false for all 64 coefficients
    assert own[names.index("flat200")].tolist() == [1 << 63] * 8               # only the DC term lies above the mean of zeros
    # the columns of a turned tile are a permutation of the tile's own: first j, then k is COMPOSE[j][k]
    for j in range(1, 8):
        block = got[j * len(tiles): (j + 1) * len(tiles)]
        for k in range(8):
            assert np.array_equal(block[:, k], own[:, turned.COMPOSE[j][k]]), (j, k)
    lr, tb, tr = (own[names.index(n)] for n in ("lr-symmetric", "tb-symmetric", "transpose-symmetric"))
    assert lr[1] == lr[0] and tb[2] == tb[0] and tr[4] == tr[0]


# ---- images -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images():
    """(images, the oracle's eight hashes per image): computed once."""
    imgs = T.hash_images()
    return imgs, [_oracle_turned(O.hash_image(px, want_tiles=True)[2]) for px in imgs]


def _by_channels(imgs):
    groups: dict = {}
    for i, px in enumerate(imgs):
        groups.setdefault(1 if px.ndim == 2 else px.shape[2], []).append(i)
    return groups


def test_hash_images_turned_in_ragged_calls(ctx, images, monkeypatch):
    """One ragged call per channel count, with the library's own group thresholds: the two 1024 x 512 images run banded."""
    monkeypatch.delenv("KE_FUSED_MIN_IMAGES", raising=False)
    imgs, want = images
    for ch, idx in _by_channels(imgs).items():
        got, status = ctx.hash_images_turned([imgs[i] for i in idx])
        assert status.tolist() == [0] * len(idx)
        plain, _, _ = ctx.hash_images([imgs[i] for i in idx], want_dhash=False)
        assert got[:, 0].tolist() == plain.tolist(), ch
        for row, i in zip(got, idx):                    # output order follows the input order
            assert row.tolist() == want[i], (ch, i, imgs[i].shape)


def test_hash_images_turned_per_shape_one_workgroup_per_image(ctx, images, monkeypatch):
    monkeypatch.setenv("KE_FUSED_MIN_IMAGES", "1")
    imgs, want = images
    shapes: dict = {}
    for i, px in enumerate(imgs):
        shapes.setdefault(px.shape, []).append(i)
    for shape, idx in shapes.items():
        got, status = ctx.hash_images_turned([imgs[i] for i in idx])
        assert status.tolist() == [0] * len(idx)
        assert got.tolist() == [want[i] for i in idx], shape


def test_hash_images_turned_on_device_resident_pixels(ctx, images, monkeypatch):
    """The RGB images packed in device memory, in reversed order: the size groups' tiles land in one scratch group after
    group and the hashes are scattered to the images' slots."""
    monkeypatch.delenv("KE_FUSED_MIN_IMAGES", raising=False)
    imgs, want = images
    idx = _by_channels(imgs)[3][::-1]
    flat, offsets, widths, heights, ch = _native._pack_images([imgs[i] for i in idx])
    dev = ctx.malloc(flat.nbytes)
    try:
        ctx.memcpy(dev, flat, flat.nbytes)
        got, status = np.zeros((len(idx), 8), np.uint64), np.zeros(len(idx), np.int32)
        ctx._check(ctx._lib.ke_hash_images_turned(ctx._h, dev, offsets.ctypes.data, widths.ctypes.data, heights.ctypes.data, ch,
                                                  len(idx), got.ctypes.data, status.ctypes.data), "ke_hash_images_turned")
    finally:
        ctx.free(dev)
    assert status.tolist() == [0] * len(idx)
    assert got.tolist() == [want[i] for i in idx]


def test_a_zero_sized_image_has_a_status_and_eight_zeros(ctx, images):
    imgs, want = images
    got, status = ctx.hash_images_turned([imgs[0], np.zeros((0, 5, 3), np.uint8), imgs[2]])
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    assert got[1].tolist() == [0] * 8
    assert got[0].tolist() == want[0] and got[2].tolist() == want[2]


def test_phash_turned_is_the_signed_row(images):
    imgs, want = images
    got = K.phash_turned(imgs[1])
    assert got == tuple(O.to_signed64(v) for v in want[1]) and got[0] == K.phash(imgs[1])


# ---- the cross scan --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """mode -> the arrays its child process wrote.  One child at a time, each under its own time limit; after one that fails,
    ends on a signal or runs into its limit, no further child is started."""
    work = tmp_path_factory.mktemp("scan_cross")
    worker = os.path.join(ROOT, "tests", "_scan_cross_worker.py")
    got = {}
    for m in MODES:
        res = subprocess.run(["timeout", "-k", "10", "180", sys.executable, worker, ROOT, str(work / f"{m}.npz")],
                             env=dict(os.environ, KE_SCAN_MODE=m), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, f"KE_SCAN_MODE={m}: exit {res.returncode}\n{res.stdout[-3000:]}"
        print(res.stdout[-300:])
        got[m] = dict(np.load(str(work / f"{m}.npz")))
        assert str(got[m]["mode"]) == m
    return got


def _oracle_rows(c):
    """(sorted edge rows of the whole table, its bucket pairs): the oracle without ids, pairs of equal id dropped afterwards."""
    exp, exp_c = O.scan_banded(c["h"], ids=None, sizes=c["sizes"], **c["kw"])
    if c["ids"] is not None:
        exp = exp[c["ids"][exp["a"]] != c["ids"][exp["b"]]]
    rows = np.stack([exp["a"].astype(np.int64), exp["b"].astype(np.int64), exp["h"].astype(np.int64), exp["bands"].astype(np.int64)],
                    axis=1).reshape(-1, 4)
    return rows[np.lexsort(rows.T[::-1])], int(exp_c[0])


@pytest.fixture(scope="module")
def truth():
    return {name: _oracle_rows(c) for name, c in CASES.items()}


def _cross(rows, f):
    return rows[(rows[:, 0] < f) & (rows[:, 1] >= f)]


def _ham(rows):
    return sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in rows[:, 3])


def test_every_cut_has_planted_pairs_on_both_sides_and_across(truth):
    """An empty answer cannot pass: for every first_new strictly inside the table some edge straddles it, and (where the cut
    leaves room) some edge lies wholly below it and some wholly above it -- the edges the cross scan must leave out."""
    rows, _ = truth["plain"]
    a, b = rows[:, 0], rows[:, 1]
    for f in S.FIRST_NEW:
        if 0 < f < S.N:
            assert ((a < f) & (b >= f)).any(), f
        if f >= 17:
            assert (b < f).any(), f
        if f <= 2048:
            assert (a >= f).any(), f
    for name in ("ids", "sizes", "cap"):
        assert len(truth[name][0]) < len(rows)


@pytest.mark.parametrize("first_new", S.FIRST_NEW)
@pytest.mark.parametrize("name", list(CASES))
def test_the_cross_region_is_the_full_scan_filtered(runs, truth, name, first_new):
    rows, bucket_pairs = truth[name]
    want = _cross(rows, first_new)
    counters = [first_new * (S.N - first_new), _ham(want), len(want), bucket_pairs]
    for m in MODES:
        got = runs[m]
        edges = got[f"{name}/{first_new}/edges"]
        assert np.array_equal(edges, want), (name, first_new, m, "oracle", len(edges), len(want))
        assert np.array_equal(edges, _cross(got[f"{name}/full/edges"], first_new)), (name, first_new, m, "ke_hamming_scan")
        assert got[f"{name}/{first_new}/counters"].tolist() == counters, (name, first_new, m)
        assert int(got[f"{name}/{first_new}/counters"][3]) == int(got[f"{name}/full/counters"][3])
    assert runs["tiles"][f"{name}/{first_new}/path"] == 0
    assert runs["buckets"][f"{name}/{first_new}/path"] == 1


def test_an_empty_side_gives_nothing(runs):
    for m in MODES:
        for name in CASES:
            for f in (0, S.N):
                assert len(runs[m][f"{name}/{f}/edges"]) == 0
                assert runs[m][f"{name}/{f}/counters"][:3].tolist() == [0, 0, 0]


def test_first_new_outside_the_table_is_refused(runs):
    for m in MODES:
        assert runs[m]["einval"].tolist() == [-1, -1]      # KE_EINVAL


@pytest.mark.parametrize("parts", S.PARTS)
@pytest.mark.parametrize("first_new", S.SHARD_FIRST_NEW)
def test_shards_partition_the_cross_region(runs, truth, first_new, parts):
    rows, bucket_pairs = truth["plain"]
    want = _cross(rows, first_new)
    assert len(want) > 0
    for m in MODES:
        got = runs[m]
        edges = got[f"shards/{first_new}/{parts}/edges"]
        assert len(edges) == len(want), (m, "an edge is missing or appears twice")
        assert np.array_equal(edges[np.lexsort(edges.T[::-1])], want), m
        cnt = got[f"shards/{first_new}/{parts}/counters"]
        assert int(cnt[:, 0].sum()) == first_new * (S.N - first_new), m
        assert int(cnt[:, 1].sum()) == _ham(want) and int(cnt[:, 2].sum()) == len(want), m
        assert cnt[:, 3].tolist() == [bucket_pairs] * parts, m
        assert len(set(got[f"shards/{first_new}/{parts}/paths"].tolist())) == 1, (m, "every shard must take the same path")


def test_a_small_edge_buffer_goes_through_the_overflow_protocol(runs, truth):
    want = _cross(truth["plain"][0], 1025)
    assert len(want) > S.SMALL_CAPACITY
    have = set(map(tuple, want.tolist()))
    for m in MODES:
        assert runs[m]["small-capacity/reported"].tolist() == [len(want), len(want)], m
        stored = runs[m]["small-capacity/stored"]
        assert len(stored) == S.SMALL_CAPACITY and set(map(tuple, stored.tolist())) <= have, m
        assert np.array_equal(runs[m]["small-capacity/grown"], want), m


def test_the_big_table_under_auto(runs):
    """n = 60 000 at first_new = 30 000 against the full scan filtered.  The path auto took is printed, not asserted."""
    got = runs["auto"]
    f = S.BIG_FIRST_NEW_WIDE
    want = _cross(got["big/full/edges"], f)
    assert 0 < len(want) < len(got["big/full/edges"])
    assert np.array_equal(got["big/cross/edges"], want)
    assert got["big/cross/counters"].tolist() == [f * (S.BIG_N - f), _ham(want), len(want), int(got["big/full/counters"][3])]
    print(f"auto path at n = {S.BIG_N}, first_new = {f}: {int(got['big/cross/path'])} (0 tiles, 1 buckets)")


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The files on disk, their DuplicateFile rows with the stored pHash (the pixels Pillow opens, hashed here), and the
    result of find_turned_duplicates: made once."""
    from PIL import Image

    folder = tmp_path_factory.mktemp("turned_files")
    records = T.write_files(folder)
    assert 38 <= len(records) <= 42
    opened = [np.asarray(Image.open(r["path"]).convert("RGB")) for r in records]
    stored, _, ok = K.hash_batch(opened, want_dhash=False)
    assert ok.all()
    files = [DuplicateFile(r["file_id"], Path(r["path"]), os.path.getsize(r["path"]), px.shape[1], px.shape[0], int(h))
             for r, px, h in zip(records, opened, stored)]
    clusters, matches = api.find_turned_duplicates(files, hamming_threshold=T.THRESHOLD)
    return dict(folder=folder, records=records, opened=opened, files=files, clusters=clusters, matches=matches)


def _planted_pairs(records) -> dict:
    """(original's id, copy's id) -> the orientation the copy was made with."""
    original = {r["picture"]: r["file_id"] for r in records if r["orientation"] == 0}
    return {(original[r["picture"]], r["file_id"]): r["orientation"] for r in records if r["orientation"]}


def test_the_planted_copies_are_within_reach_by_the_oracle_alone(library):
    """Every copy's pHash (of the pixels Pillow opens, JPEG loss included) lies within the threshold of, and shares a 16-bit
    band with, the turned hash of the PNG original's tile for the orientation the copy was made with."""
    records, opened = library["records"], library["opened"]
    at = {r["file_id"]: i for i, r in enumerate(records)}
    pairs = _planted_pairs(records)
    assert len(pairs) == 10 and sorted(set(pairs.values())) == [1, 2, 3, 5, 6]
    for (orig, copy), k in pairs.items():
        tile = O.hash_image(opened[at[orig]], want_tiles=True)[2]
        from_tile = O.phash_from_tile(T.turn_k(k, tile))[0]
        of_copy = O.hash_image(opened[at[copy]])[0]
        d = O.hamming64(from_tile, of_copy)
        shared = [b for b in range(4) if (from_tile >> (16 * b)) & 0xFFFF == (of_copy >> (16 * b)) & 0xFFFF]
        assert d <= T.THRESHOLD and shared, (records[at[copy]]["path"], k, d, shared)


def test_the_stored_hashes_alone_link_no_planted_pair(library):
    clusters = api.find_duplicates(library["files"], hamming_threshold=T.THRESHOLD)
    for c in clusters:
        members = {e.file.file_id for e in c.files}
        for pair in _planted_pairs(library["records"]):
            assert not set(pair) <= members, pair


def test_find_turned_duplicates_links_every_planted_pair_and_nothing_else(library):
    pairs = _planted_pairs(library["records"])
    got = {(m.file_id_a, m.file_id_b): m for m in library["matches"]}
    assert all(isinstance(m, TurnedMatch) and m.file_id_a < m.file_id_b for m in library["matches"])
    # the orientation turns the copy's picture (the larger id) back into the original's
    assert {pair: m.orientation for pair, m in got.items()} == {pair: turned.INVERSE[k] for pair, k in pairs.items()}
    assert all(m.hamming <= T.THRESHOLD for m in got.values())
    groups = {frozenset(e.file.file_id for e in c.files) for c in library["clusters"]}
    by_original: dict = {}
    for (orig, copy) in pairs:
        by_original.setdefault(orig, {orig}).add(copy)
    assert groups == {frozenset(v) for v in by_original.values()}           # the untouched files stay alone


def test_turned_signatures_are_the_oracles_on_the_files_pixels(library):
    sig, ok = turned.turned_signatures([r["path"] for r in library["records"]] + [str(library["folder"] / "missing.png")])
    assert ok.tolist() == [True] * len(library["records"]) + [False] and sig[-1].tolist() == [0] * 8
    for row, px in zip(sig, library["opened"]):
        assert row.tolist() == _oracle_turned(O.hash_image(px, want_tiles=True)[2])


def test_scan_dups_turned_lists_the_same_links(library, tmp_path, capsys):
    records, files = library["records"], library["files"]
    db = str(tmp_path / "k.db")
    conn = sqlite3.connect(db)
    conn.execute("CREATE TABLE files (id INTEGER PRIMARY KEY, path TEXT, size INTEGER, width INTEGER, height INTEGER, is_present INTEGER)")
    conn.execute("CREATE TABLE signatures (file_id INTEGER PRIMARY KEY, phash_u64 INTEGER, dhash_u64 INTEGER)")
    for f in files:
        conn.execute("INSERT INTO files VALUES (?, ?, ?, ?, ?, 1)", (f.file_id, str(f.path), f.size, f.width, f.height))
        conn.execute("INSERT INTO signatures VALUES (?, ?, 0)", (f.file_id, O.to_signed64(f.phash)))
    conn.commit()
    conn.close()
    out_csv = str(tmp_path / "out.csv")
    assert cli.main(["scan-dups", "--db", db, "--turned", "--csv", out_csv]) == 0
    assert "5 duplicate group(s), 15 file(s)" in capsys.readouterr().out
    with open(out_csv, newline="") as handle:
        rows = list(csv.DictReader(handle))
    assert list(rows[0]) == cli.CSV_HEADER + ["orientation"]
    groups: dict = {}
    for r in rows:
        groups.setdefault(r["group"], []).append(r)
    assert {frozenset(int(r["file_id"]) for r in g) for g in groups.values()} == \
        {frozenset(e.file.file_id for e in c.files) for c in library["clusters"]}
    made_with = {r["file_id"]: r["orientation"] for r in records}
    for g in groups.values():
        keeper = next(int(r["file_id"]) for r in g if r["keeper"] == "1")
        for r in g:
            # the file is orientation x of the picture, the keeper orientation kk: undo x, then apply kk
            want = turned.COMPOSE[turned.INVERSE[made_with[int(r["file_id"])]]][made_with[keeper]]
            assert r["orientation"] == (str(want) if want else ""), (r["path"], keeper)
    # without the flag the command does what it did: no orientation column, the copies of one picture only
    assert cli.main(["scan-dups", "--db", db, "--csv", out_csv]) == 0
    with open(out_csv, newline="") as handle:
        plain = list(csv.DictReader(handle))
    assert list(plain[0]) == cli.CSV_HEADER and len(plain) == 10
