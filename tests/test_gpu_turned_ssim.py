"""The SSIM re-check of turned pairs on the device.

1. ke_turn_luma over one mixed batch == turn(k, O.luma(px)) byte for byte, guard bytes behind every plane untouched.
2. ke_ssim_pairs_turned(a, b, k) is bit-equal (float64 ==, same status) to ke_ssim_pairs on a and a host-made turn(k, b):
   luma commutes with the turn and every resample plan is pinned bit-exact, so there is no tolerance.
3. ke_ssim_pairs_turned against the oracle's ssim_fit(a, turn(k, b)): 1e-5 in the default mode, 1e-6 in the exact one --
   the bars of tests/test_gpu_parity.py.
4. refine_turned_pairs at the seam: PNG and JPEG files, a wrong orientation, a file no decoder takes.
5. find_turned_duplicates(ssim_threshold=...) and scan-dups --turned --turned-ssim on a small corpus with decoys whose
   pHash survives Gaussian noise of sigma 40 and whose SSIM does not."""
from __future__ import annotations

import csv
import os
import sqlite3
from pathlib import Path

import numpy as np
import pytest

import _turned_cases as T
import _turned_ssim_cases as S
import kobato_eyes_amd as K
from kobato_eyes_amd import _native, api, cli, refine, turned
from kobato_eyes_amd.scanner import DuplicateFile
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _native.get_context(0)


def _turn(k, a):
    return np.ascontiguousarray(turned.turn(k, a))


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
GUARD = 16


def test_turn_luma_on_a_mixed_batch(ctx):
    assert S.TILE == 64 and any(w > 3 * S.TILE and h > 3 * S.TILE for w, h in S.KERNEL_SHAPES)
    rng = np.random.default_rng(S.SEED)
    sources, src_off, at = [], [], 0
    for w, h in S.KERNEL_SHAPES:                        # packed back to back: a 1 x 1 grey image puts the rest off the dwords
        for ch in (1, 3, 4):
            px = rng.integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
            sources.append(px)
            src_off.append(at)
            at += px.size
    assert {o % 4 for o in src_off} == {0, 1, 2, 3}
    flat = np.concatenate([px.reshape(-1) for px in sources])
    jobs = [(i, k) for i in range(len(sources)) for k in range(8)]
    want = [_turn(k, O.luma(sources[i])) for i, k in jobs]
    assert {p.shape[1] % 4 for p in want} == {0, 1, 2, 3}            # destination widths of every residue
    dst_off, at = [], 3                                              # planes packed too, 16 guard bytes behind each
    for p in want:
        dst_off.append(at)
        at += p.size + GUARD
    assert {o % 4 for o in dst_off} == {0, 1, 2, 3}
    total = at
    src, dst = ctx.malloc(flat.nbytes), ctx.malloc(total)
    try:
        ctx.memcpy(src, flat, flat.nbytes)
        ctx.memcpy(dst, np.full(total, 0xA5, np.uint8), total)
        ctx.turn_luma(src, [src_off[i] for i, _ in jobs], [sources[i].shape[1] for i, _ in jobs], [sources[i].shape[0] for i, _ in jobs],
                      [1 if sources[i].ndim == 2 else sources[i].shape[2] for i, _ in jobs], [k for _, k in jobs], dst, dst_off)
        got = np.empty(total, np.uint8)
        ctx.memcpy(got, dst, total)
    finally:
        ctx.free(src)
        ctx.free(dst)
    assert np.all(got[:3] == 0xA5)
    for (i, k), p, o in zip(jobs, want, dst_off):
        assert np.array_equal(got[o:o + p.size].reshape(p.shape), p), (sources[i].shape, k)
        assert np.all(got[o + p.size:o + p.size + GUARD] == 0xA5), (sources[i].shape, k)


def test_turn_luma_refuses_what_it_cannot_take(ctx):
    dev = ctx.malloc(64)
    try:
        for w, h, ch, k in ((4, 4, 3, 8), (4, 4, 3, -1), (4, 4, 2, 0), (0, 4, 3, 0)):
            with pytest.raises(ValueError):
                ctx.turn_luma(dev, [0], [w], [h], [ch], [k], dev, [0])
    finally:
        ctx.free(dev)


# ---- 2. and 3. the library call -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    """The images of PAIR_SHAPES (a_0, b_0, a_1, b_1, ...), the (a, b, k) rows -- every pair under every orientation, and
    b_0 once as somebody's a --, the host-turned images and the oracle's scores: made once."""
    images = []
    for n, (sa, sb) in enumerate(S.PAIR_SHAPES):
        a = T.picture(S.SEED + 200 + n, sa[0], sa[1], 3)
        # b: the picture itself brought to b's shape by a crop or a turn, under light noise, so that the scores are not all alike
        b = T.picture(S.SEED + 200 + n, sb[0], sb[1], 3) if n != 0 else S.noisy(T.turn_k(5, a), S.SEED + 250, 6.0)
        assert (b.shape[1], b.shape[0]) == sb
        images += [a, b]
    rows = [(2 * n, 2 * n + 1, k) for n in range(len(S.PAIR_SHAPES)) for k in range(8)]
    rows += [(1, 0, 6), (1, 2, 0)]                       # b_0, turned under eight orientations above, is an a here
    host = [_turn(k, images[b]) for _, b, k in rows]
    oracle = [O.ssim_fit(images[a], t) for (a, _, _), t in zip(rows, host)]
    return dict(images=images, rows=rows, host=host, oracle=oracle)


def _turned_call(ctx, p):
    a, b, k = (list(col) for col in zip(*p["rows"]))
    return ctx.ssim_pairs_turned(p["images"], a, b, k)


def test_ssim_pairs_turned_is_ssim_pairs_on_the_host_turned_image(ctx, pairs):
    rows, images, host = pairs["rows"], pairs["images"], pairs["host"]
    got, status = _turned_call(ctx, pairs)
    n = len(images)
    want, want_status = ctx.ssim_pairs(images + host, [a for a, _, _ in rows], [n + j for j in range(len(rows))])
    for row, g, w, gs, ws in zip(rows, got.tolist(), want.tolist(), status.tolist(), want_status.tolist()):
        print(row, g, w)
        assert gs == ws == 0 and g == w, row
    # b_0 is a_0 turned clockwise (5) under light noise: the counter-clockwise turn (6) brings it back, and only that one
    # (the oracle, on the CPU: 0.913 against at most 0.463 for the other seven)
    assert got[rows.index((0, 1, 6))] > 0.9 and all(got[rows.index((0, 1, k))] < 0.5 for k in range(8) if k != 6)
    # statuses mean what they mean: a common size under 7, an index outside the images
    small = [images[0], np.zeros((5, 30, 3), np.uint8)]
    sc, st = ctx.ssim_pairs_turned(small, [0, 0, 0], [1, 1, 7], [0, 4, 0])
    assert st.tolist() == [1, 1, 2] and np.isnan(sc).all()
    assert ctx.ssim_pairs_turned([images[0], np.zeros((30, 5, 3), np.uint8)], [0], [1], [4])[1].tolist() == [1]   # 30 x 5 turned: 5 x 30


def test_all_zero_orientations_are_ssim_pairs(ctx, pairs):
    images = pairs["images"]
    a = [0, 2, 4, 6, 1, 0]
    b = [1, 3, 5, 7, 0, 0]
    want, want_status = ctx.ssim_pairs(images, a, b)
    for orient in ([0] * len(a), None):
        got, status = ctx.ssim_pairs_turned(images, a, b, orient)
        assert got.tolist() == want.tolist() and status.tolist() == want_status.tolist()


def test_an_orientation_outside_0_to_7_fails_the_call(ctx, pairs):
    for bad in (8, -1):
        with pytest.raises(ValueError, match="orientation"):
            ctx.ssim_pairs_turned(pairs["images"], [0, 0], [1, 1], [3, bad])


def test_ssim_pairs_turned_against_the_oracle(ctx, pairs):
    got, _ = _turned_call(ctx, pairs)
    ctx.ssim_set_mode(True)
    try:
        exact, _ = _turned_call(ctx, pairs)
    finally:
        ctx.ssim_set_mode(False)
    for row, g, e, w in zip(pairs["rows"], got.tolist(), exact.tolist(), pairs["oracle"]):
        print(row, g, e, w)
        assert abs(g - w) <= 1e-5, row
        assert abs(e - w) <= 1e-6, row


# ---- 4. the seam ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", ["png", "jpg"])
def test_refine_turned_pairs_at_the_seam(ctx, tmp_path, ext):
    from PIL import Image

    px = T.picture(S.SEED + 500, 96, 80, 3)
    how = {"quality": 95} if ext == "jpg" else {}
    path_a = str(tmp_path / f"a.{ext}")
    Image.fromarray(px).save(path_a, **how)
    a = np.asarray(Image.open(path_a).convert("RGB"))
    turned_rows, plain_rows, wrong_rows, loader_rows = [], [], [], []
    for k in range(8):
        # b_k holds orientation INVERSE[k] of the picture, written with Pillow's own transpose: orientation k of it is the picture
        name = turned.ORIENTATIONS[turned.INVERSE[k]][1]
        im = Image.fromarray(px)
        path_b = str(tmp_path / f"b{k}.{ext}")
        (im.transpose(getattr(Image.Transpose, name)) if name else im).save(path_b, **how)
        with Image.open(path_b) as opened:
            b = opened.convert("RGB")
            b.load()
        # the file refine_pairs sees: what Pillow reads from b_k, turned by Pillow, stored without loss
        name = turned.ORIENTATIONS[k][1]
        path_c = str(tmp_path / f"c{k}.png")
        (b.transpose(getattr(Image.Transpose, name)) if name else b).save(path_c)
        path_ppm = str(tmp_path / f"b{k}.ppm")              # no GPU decoder takes a PPM file: the loader's route
        b.save(path_ppm)
        wrong = (k + 1) % 8
        assert O.ssim_fit(a, _turn(wrong, np.asarray(b))) < 0.5
        turned_rows.append((1, 10 + k, path_a, path_b, k))
        plain_rows.append((1, 10 + k, path_a, path_c))
        wrong_rows.append((1, 10 + k, path_a, path_b, wrong))
        loader_rows.append((1, 10 + k, path_a, path_ppm, k))
    cfg = refine.RefinementThresholds(ssim=0.9)
    stats: dict = {}
    got = refine.refine_turned_pairs(turned_rows, thresholds=cfg, stats=stats)
    want = refine.refine_pairs(plain_rows, thresholds=cfg)
    assert stats["pairs"] == 8 and stats["decodes"] == 9
    for k, (g, w) in enumerate(zip(got, want)):
        print(ext, k, g.ssim, w.ssim)
        assert g == w and g.is_duplicate and (g.file_id_a, g.file_id_b) == (1, 10 + k), k     # dataclass equality: the float compared with ==
    assert all(m.ssim < 0.5 and not m.is_duplicate for m in refine.refine_turned_pairs(wrong_rows, thresholds=cfg))
    by_loader: dict = {}
    assert refine.refine_turned_pairs(loader_rows, thresholds=cfg, stats=by_loader) == got
    assert by_loader["decodes"] == 9 and by_loader["gpu_decodes"] <= 1          # at most a itself was decoded on the device
    # an unreadable file gives None, in place
    missing = refine.refine_turned_pairs([turned_rows[1], (1, 99, path_a, str(tmp_path / "absent.png"), 3), turned_rows[5]], thresholds=cfg)
    assert missing[1] is None and missing[0] == got[1] and missing[2] == got[5]
    with pytest.raises(ValueError):
        refine.refine_turned_pairs([(1, 2, path_a, path_a, 8)])


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    folder = tmp_path_factory.mktemp("turned_ssim_files")
    records = S.write_corpus(folder)
    stored, _, ok = K.hash_batch([r["px"] for r in records], want_dhash=False)
    assert ok.all()
    files = [DuplicateFile(r["file_id"], Path(r["path"]), os.path.getsize(r["path"]), r["px"].shape[1], r["px"].shape[0], int(h))
             for r, h in zip(records, stored)]
    baseline = api.find_turned_duplicates(files, hamming_threshold=T.THRESHOLD)
    return dict(folder=folder, records=records, files=files, baseline=baseline)


def _groups(clusters):
    return {frozenset(e.file.file_id for e in c.files) for c in clusters}


def test_find_turned_duplicates_with_an_ssim_threshold(corpus, tmp_path, capsys):
    records, files = corpus["records"], corpus["files"]
    by_id = {r["file_id"]: r for r in records}
    decoys = {r["file_id"] for r in records if r["decoy"]}
    base_clusters, base_matches = corpus["baseline"]
    # preconditions.  By the oracle alone every decoy is within reach of the scan and scores under 0.5 against every
    # orientation of every file of its picture ...
    assert len(decoys) == 3 and set(S.decoy_reach(O, records)) == decoys
    for d in decoys:
        for r in records:
            if r["picture"] == by_id[d]["picture"] and not r["decoy"]:
                assert max(O.ssim_fit(r["px"], _turn(k, by_id[d]["px"])) for k in range(8)) < 0.5
    # ... and without ssim_threshold the hashes do link each: what this route gave before it could look at the pixels
    linked = {f for m in base_matches for f in (m.file_id_a, m.file_id_b)}
    assert decoys <= linked and all(m.ssim is None for m in base_matches)
    true_pairs = {(m.file_id_a, m.file_id_b) for m in base_matches if not {m.file_id_a, m.file_id_b} & decoys}
    originals = {r["picture"]: r["file_id"] for r in records if not r["decoy"] and r["orientation"] == 0}
    for r in records:                                               # every planted copy is linked to its original
        if not r["decoy"] and r["orientation"]:
            assert (originals[r["picture"]], r["file_id"]) in true_pairs
    families = {frozenset(r["file_id"] for r in records if r["picture"] == i and not r["decoy"]) for i in range(len(S.CORPUS))}
    assert any(g & decoys for g in _groups(base_clusters))

    clusters, matches = api.find_turned_duplicates(files, hamming_threshold=T.THRESHOLD, ssim_threshold=0.9)
    assert {(m.file_id_a, m.file_id_b) for m in matches} == true_pairs and len(matches) == len(true_pairs)
    assert _groups(clusters) == families
    rows = [(m.file_id_a, m.file_id_b, by_id[m.file_id_a]["path"], by_id[m.file_id_b]["path"], m.orientation) for m in matches]
    refined = refine.refine_turned_pairs(rows, thresholds=refine.RefinementThresholds(ssim=0.9))
    for m, r in zip(matches, refined):
        want = O.ssim_fit(by_id[m.file_id_a]["px"], _turn(m.orientation, by_id[m.file_id_b]["px"]))
        print(m, want)
        assert m.ssim == r.ssim and m.ssim >= 0.9 and abs(m.ssim - want) <= 1e-5
        assert (m.orientation, m.hamming) == next((b.orientation, b.hamming) for b in base_matches
                                                  if (b.file_id_a, b.file_id_b) == (m.file_id_a, m.file_id_b))

    everything, all_matches = api.find_turned_duplicates(files, hamming_threshold=T.THRESHOLD, ssim_threshold=0.0)
    assert [(m.file_id_a, m.file_id_b, m.orientation, m.hamming) for m in all_matches] == \
        [(m.file_id_a, m.file_id_b, m.orientation, m.hamming) for m in base_matches]
    assert all(m.ssim is not None for m in all_matches) and _groups(everything) == _groups(base_clusters)
    again = api.find_turned_duplicates(files, hamming_threshold=T.THRESHOLD, ssim_threshold=None)
    assert again[1] == base_matches and _groups(again[0]) == _groups(base_clusters)

    # the command line: the same groups, and the orientation column worked out from the survivors
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
    assert cli.main(["scan-dups", "--db", db, "--turned", "--turned-ssim", "0.9", "--csv", out_csv]) == 0
    assert f"{len(families)} duplicate group(s), {sum(map(len, families))} file(s)" in capsys.readouterr().out
    with open(out_csv, newline="") as handle:
        table = list(csv.DictReader(handle))
    assert list(table[0]) == cli.CSV_HEADER + ["orientation"]
    groups: dict = {}
    for row in table:
        groups.setdefault(row["group"], []).append(row)
    assert {frozenset(int(r["file_id"]) for r in g) for g in groups.values()} == families
    for g in groups.values():
        keeper = next(int(r["file_id"]) for r in g if r["keeper"] == "1")
        for r in g:
            # the file is orientation x of the picture, the keeper orientation kk: undo x, then apply kk
            want = turned.COMPOSE[turned.INVERSE[by_id[int(r["file_id"])]["orientation"]]][by_id[keeper]["orientation"]]
            assert r["orientation"] == (str(want) if want else ""), (r["path"], keeper)
