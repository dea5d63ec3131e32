"""The SSIM re-check of trimmed pairs on the device.

1. ke_crop_luma over one mixed batch == O.luma(px)[y0:y1, x0:x1] byte for byte, guard bytes round every plane untouched.
2. ke_ssim_pairs_boxed(a, b, box_a, box_b) is bit-equal (float64 ==, same status) to ke_ssim_pairs on host-made crops: luma
   is per pixel and every resample plan is pinned bit-exact, so there is no tolerance.  Against the oracle's ssim_fit of the
   crops: 1e-5 in the default mode, 1e-6 in the exact one -- the bars of tests/test_gpu_parity.py.
3. refine_trimmed_pairs at the seam: PNG and JPEG files of every border kind, flags off, a file no decoder takes, a missing
   file, a picture without a box, and a JPEG with an EXIF orientation, whose box on the file as it lies would not fit.
4. find_trimmed_duplicates(ssim_threshold=...) and scan-dups --trimmed --trimmed-ssim on _trimmed_ssim_cases' corpus, whose
   decoys the trimmed pHash links and the pixels do not (tests/test_trimmed_ssim_cpu.py holds the corpus to that)."""
from __future__ import annotations

import csv
import os
import sqlite3
from pathlib import Path

import numpy as np
import pytest

import _trim_cases as T
import _trimmed_ssim_cases as S
import _turned_cases as TC
import _turned_ssim_cases as TS
import kobato_eyes_amd as K
from kobato_eyes_amd import _native, api, cli, refine
from kobato_eyes_amd.scanner import DuplicateFile
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _native.get_context(0)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
BEHIND, FRONT = 16, 3


def test_crop_luma_on_a_mixed_batch(ctx):
    rng = np.random.default_rng(T.SEED + 800)
    sources, src_off, at = [], [], 0
    for w, h in S.KERNEL_SHAPES:                        # packed back to back: a 1 x 1 grey image puts the rest off the dwords
        for ch in (1, 3, 4):
            px = rng.integers(0, 256, size=(h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
            sources.append(px)
            src_off.append(at)
            at += px.size
    assert {o % 4 for o in src_off} == {0, 1, 2, 3}
    flat = np.concatenate([px.reshape(-1) for px in sources])
    chans = [1 if px.ndim == 2 else px.shape[2] for px in sources]
    jobs = [(i, box) for i, px in enumerate(sources) for box in S.kernel_boxes(px.shape[1], px.shape[0])]
    lumas = [O.luma(px) for px in sources]
    want = [np.ascontiguousarray(lumas[i][y0:y1, x0:x1]) for i, (x0, y0, x1, y1) in jobs]
    dst_off, at = [], FRONT                                          # planes packed too, 16 guard bytes behind each
    for p in want:
        dst_off.append(at)
        at += p.size + BEHIND
    total = at
    # what the batch is made to hold: every residue mod 4 of the box's first source byte (through x0 * ch, and through the
    # image's own offset), of the box's width and of the plane's address; the first and the last byte of an image; and a box
    # taller than four rows for every wave of the launch, so that a wave walks on through its row loop
    for ch in (1, 3):
        assert {(box[0] * chans[i]) % 4 for i, box in jobs if chans[i] == ch} == {0, 1, 2, 3}
    assert {(src_off[i] + box[0] * chans[i]) % 4 for i, box in jobs} == {0, 1, 2, 3}
    assert {(box[2] - box[0]) % 4 for _, box in jobs} == {0, 1, 2, 3} == {o % 4 for o in dst_off}
    for i, px in enumerate(sources):
        h, w = px.shape[:2]
        assert (i, (0, 0, 1, 1)) in jobs and (i, (w - 1, h - 1, w, h)) in jobs and (i, (0, 0, w, h)) in jobs
    tallest = max(box[3] - box[1] for _, box in jobs)
    waves = 4 * min(max((tallest + S.ROWS_PER_BLOCK - 1) // S.ROWS_PER_BLOCK, 1), 256)
    assert tallest > 4 * waves and sum(box[3] - box[1] > 4 * waves for _, box in jobs) >= 6
    src, dst = ctx.malloc(flat.nbytes), ctx.malloc(total)
    try:
        assert src % 4 == 0 and dst % 4 == 0
        ctx.memcpy(src, flat, flat.nbytes)
        ctx.memcpy(dst, np.full(total, 0xA5, np.uint8), total)
        ctx.crop_luma(src, [src_off[i] for i, _ in jobs], [sources[i].shape[1] for i, _ in jobs], [sources[i].shape[0] for i, _ in jobs],
                      [chans[i] for i, _ in jobs], [box for _, box in jobs], dst, dst_off)
        assert ctx.last_kernel_ms(7) >= 0.0
        got = np.empty(total, np.uint8)
        ctx.memcpy(got, dst, total)
    finally:
        ctx.free(src)
        ctx.free(dst)
    assert np.all(got[:FRONT] == 0xA5)
    for (i, box), p, o in zip(jobs, want, dst_off):
        assert np.array_equal(got[o:o + p.size].reshape(p.shape), p), (sources[i].shape, box)
        assert np.all(got[o + p.size:o + p.size + BEHIND] == 0xA5) and np.all(got[o - FRONT:o] == 0xA5), (sources[i].shape, box)


def test_crop_luma_refuses_what_it_cannot_take(ctx):
    dev = ctx.malloc(256)
    try:
        for w, h, ch, box in ((6, 5, 3, (2, 1, 2, 4)), (6, 5, 3, (0, 3, 4, 3)), (6, 5, 3, (0, 0, 7, 5)), (6, 5, 3, (0, 0, 6, 6)),
                              (6, 5, 3, (-1, 0, 3, 3)), (6, 5, 2, (0, 0, 3, 3)), (0, 5, 3, (0, 0, 1, 1))):
            with pytest.raises(ValueError):
                ctx.crop_luma(dev, [0], [w], [h], [ch], [box], dev + 128, [0])
        ctx.crop_luma(dev, [], [], [], [], np.zeros((0, 4), np.int32), dev, [])              # nothing to do is no error
    finally:
        ctx.free(dev)


# ---- 2. the library call ---------------------------------------------------------------------------------------------------------
def _boxes_of(w: int, h: int) -> tuple:
    """Two boxes of a w x h picture: margins of different, odd sizes on every side; a cut off the left and the right alone."""
    return (w // 8 + 1, h // 10, w - w // 6, h - h // 12 - 1), (3, 0, w - 5, h)


@pytest.fixture(scope="module")
def pairs():
    """The images of _turned_ssim_cases.PAIR_SHAPES (a_0, b_0, a_1, b_1, ...) and the rows (a, b, box_a, box_b), None for the
    image as it lies: per pair a box on a only, on b only and on both, and every image boxed two ways in one call.  The
    host-made crops and the oracle's scores: made once."""
    images = []
    for n, (sa, sb) in enumerate(TS.PAIR_SHAPES):
        a = TC.picture(TS.SEED + 600 + n, sa[0], sa[1], 3)
        b = TS.noisy(TC.picture(TS.SEED + 600 + n, sb[0], sb[1], 3), TS.SEED + 650 + n, 6.0)
        images += [a, b]
    rows = []
    for n, (sa, sb) in enumerate(TS.PAIR_SHAPES):
        (a1, a2), (b1, b2) = _boxes_of(*sa), _boxes_of(*sb)
        rows += [(2 * n, 2 * n + 1, a1, None), (2 * n, 2 * n + 1, None, b1), (2 * n, 2 * n + 1, a2, b2), (2 * n, 2 * n + 1, a2, b1),
                 (2 * n + 1, 2 * n, b2, None)]
    rows.append((0, 0, _boxes_of(96, 80)[0], _boxes_of(96, 80)[1]))                      # one image against itself, boxed two ways
    cut = lambda i, box: images[i] if box is None else T.crop(images[i], box)
    crops = [(cut(a, ba), cut(b, bb)) for a, b, ba, bb in rows]
    oracle = [O.ssim_fit(ca, cb) for ca, cb in crops]
    return dict(images=images, rows=rows, crops=crops, oracle=oracle)


def _columns(rows) -> tuple:
    zero = (0, 0, 0, 0)
    return ([r[0] for r in rows], [r[1] for r in rows], [r[2] or zero for r in rows], [r[3] or zero for r in rows])


def test_ssim_pairs_boxed_is_ssim_pairs_on_the_host_made_crops(ctx, pairs):
    rows = pairs["rows"]
    got, status = ctx.ssim_pairs_boxed(pairs["images"], *_columns(rows))
    flat = [c for two in pairs["crops"] for c in two]
    want, want_status = ctx.ssim_pairs(flat, list(range(0, len(flat), 2)), list(range(1, len(flat), 2)))
    for row, g, w, gs, ws in zip(rows, got.tolist(), want.tolist(), status.tolist(), want_status.tolist()):
        print(row, g, w)
        assert gs == ws == 0 and g == w, row
    assert len(set(got.tolist())) > len(rows) // 2                                       # the boxes change the scores: not all alike


def test_whole_boxes_are_ssim_pairs(ctx, pairs):
    images = pairs["images"]
    a = [0, 2, 4, 6, 1, 0]
    b = [1, 3, 5, 7, 0, 0]
    want, want_status = ctx.ssim_pairs(images, a, b)
    assert not want_status.any()
    zeros = np.zeros((len(a), 4), np.int32)
    size = lambda idx: np.array([(0, 0, images[i].shape[1], images[i].shape[0]) for i in idx], np.int32)
    for box_a, box_b in ((None, None), (zeros, zeros), (size(a), size(b)), (None, size(b)), (zeros, None)):
        got, status = ctx.ssim_pairs_boxed(images, a, b, box_a, box_b)
        assert got.tolist() == want.tolist() and status.tolist() == want_status.tolist()


def test_ssim_pairs_boxed_against_the_oracle(ctx, pairs):
    got, _ = ctx.ssim_pairs_boxed(pairs["images"], *_columns(pairs["rows"]))
    ctx.ssim_set_mode(True)
    try:
        exact, _ = ctx.ssim_pairs_boxed(pairs["images"], *_columns(pairs["rows"]))
    finally:
        ctx.ssim_set_mode(False)
    for row, g, e, w in zip(pairs["rows"], got.tolist(), exact.tolist(), pairs["oracle"]):
        print(row, g, e, w)
        assert abs(g - w) <= 1e-5, row
        assert abs(e - w) <= 1e-6, row


def test_statuses_and_a_box_outside_its_image(ctx, pairs):
    images = pairs["images"][:2]                                                       # 96 x 80 and 80 x 96
    zero = (0, 0, 0, 0)
    # a box that leaves a common side under 7; an index outside the images, whatever its box says
    sc, st = ctx.ssim_pairs_boxed(images, [0, 0, 0, 1], [1, 1, 7, 0], [(5, 5, 11, 60), zero, zero, (0, 0, 80, 6)],
                                  [zero, (0, 0, 80, 6), (9, 9, 9, 9), zero])
    assert st.tolist() == [1, 1, 2, 1] and np.isnan(sc).all()
    for bad in ((0, 0, 97, 80), (10, 0, 10, 80), (-1, 0, 50, 50), (0, 0, 96, 81), (0, 0, 0, 5)):
        with pytest.raises(ValueError, match="pair 1"):
            ctx.ssim_pairs_boxed(images, [0, 0], [1, 1], [zero, bad], [zero, zero])
    with pytest.raises(ValueError, match="pair 0"):
        ctx.ssim_pairs_boxed(images, [0], [1], None, [(0, 0, 81, 96)])


# ---- 3. the seam ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", ["png", "jpg"])
def test_refine_trimmed_pairs_at_the_seam(ctx, tmp_path, ext):
    from PIL import Image

    px = T.originals()[1]
    how = {"quality": 95} if ext == "jpg" else {}
    path_a = str(tmp_path / f"a.{ext}")
    Image.fromarray(px).save(path_a, **how)
    trimmed_rows, crop_rows, off_rows, whole_rows, loader_rows = [], [], [], [], []
    for k, kind in enumerate(T.BORDER_KINDS):
        path_b = str(tmp_path / f"b{k}.{ext}")
        Image.fromarray(T.bordered(px, kind)[0]).save(path_b, **how)
        with Image.open(path_b) as opened:
            b = opened.convert("RGB")
            b.load()
        box = T.content_box(np.asarray(b), T.TOLERANCE)
        assert T.qualifies(b.width, b.height, box)
        # the file refine_pairs sees: Pillow's crop of what Pillow reads from b_k, stored without loss
        path_c = str(tmp_path / f"c{k}.png")
        b.crop(box).save(path_c)
        path_ppm = str(tmp_path / f"b{k}.ppm")              # no GPU decoder takes a PPM file: the loader's route
        b.save(path_ppm)
        trimmed_rows.append((1, 10 + k, path_a, path_b, False, True))
        crop_rows.append((1, 10 + k, path_a, path_c))
        off_rows.append((1, 10 + k, path_a, path_b, False, False))
        whole_rows.append((1, 10 + k, path_a, path_b))
        loader_rows.append((1, 10 + k, path_a, path_ppm, False, True))
    cfg = refine.RefinementThresholds(ssim=0.9)
    stats: dict = {}
    got = refine.refine_trimmed_pairs(trimmed_rows, thresholds=cfg, stats=stats)
    want = refine.refine_pairs(crop_rows, thresholds=cfg)
    assert (stats["pairs"], stats["decodes"], stats["box_files"], stats["crop_launches"]) == (4, 5, 4, 1)
    for k, (g, w) in enumerate(zip(got, want)):
        print(ext, k, g.ssim, w.ssim)
        assert g == w and g.is_duplicate and (g.file_id_a, g.file_id_b) == (1, 10 + k), k     # dataclass equality: the float compared with ==
    # the flags off: the whole files, as refine_pairs scores them -- and the asymmetric margins then hide the copy
    off_stats: dict = {}
    off = refine.refine_trimmed_pairs(off_rows, thresholds=cfg, stats=off_stats)
    assert off == refine.refine_pairs(whole_rows, thresholds=cfg)
    assert (off_stats["box_files"], off_stats["crop_launches"]) == (0, 0)
    assert not off[list(T.BORDER_KINDS).index("white margins")].is_duplicate
    # the bordered file first: the flag belongs to its side
    swapped = refine.refine_trimmed_pairs([(fb, fa, pb, pa, tb, ta) for fa, fb, pa, pb, ta, tb in trimmed_rows], thresholds=cfg)
    assert swapped == refine.refine_pairs([(fb, fa, pc, pa) for fa, fb, pa, pc in crop_rows], thresholds=cfg)
    by_loader: dict = {}
    assert refine.refine_trimmed_pairs(loader_rows, thresholds=cfg, stats=by_loader) == got
    assert by_loader["decodes"] == 5 and by_loader["gpu_decodes"] <= 1          # at most a itself was decoded on the device
    # an unreadable file gives None, in place
    missing = refine.refine_trimmed_pairs([trimmed_rows[1], (1, 99, path_a, str(tmp_path / "absent.png"), False, True), trimmed_rows[3]],
                                          thresholds=cfg)
    assert missing[1] is None and missing[0] == got[1] and missing[2] == got[3]
    # a flagged side whose picture has no box at the seam is scored as it lies
    path_flat = str(tmp_path / "flat.png")
    Image.fromarray(np.full((96, 128, 3), 90, np.uint8)).save(path_flat)
    assert refine.refine_trimmed_pairs([(1, 50, path_a, path_flat, False, True)], thresholds=cfg) == \
        refine.refine_pairs([(1, 50, path_a, path_flat)], thresholds=cfg)
    with pytest.raises(ValueError):
        refine.refine_trimmed_pairs(trimmed_rows, tolerance=256)


@pytest.mark.parametrize("kind", ["letterbox", "white margins"])
def test_the_seam_finds_its_own_box_under_an_exif_orientation(ctx, tmp_path, kind):
    """The reason the seam makes its own boxes: the loader turns the picture, so the box of the file as it lies is one of
    another pixel grid."""
    from PIL import Image

    px = T.originals()[5]                                               # 120 x 160
    pic, placed = T.bordered(px, kind)
    path_a, path_b = str(tmp_path / "upright.png"), str(tmp_path / "turned.jpg")
    Image.fromarray(px).save(path_a)
    exif = Image.Exif()
    exif[0x0112] = 6                                                    # shown turned a quarter clockwise: stored a quarter the other way
    Image.fromarray(pic).transpose(Image.Transpose.ROTATE_90).save(path_b, quality=95, exif=exif)
    as_it_lies = np.asarray(Image.open(path_b).convert("RGB"))
    assert as_it_lies.shape[:2] == (pic.shape[1], pic.shape[0])
    lying_box = T.content_box(as_it_lies, T.TOLERANCE)
    assert lying_box[2] > pic.shape[1] or lying_box[3] > pic.shape[0]   # it does not fit the picture the seam compares
    stats: dict = {}
    got = refine.refine_trimmed_pairs([(1, 2, path_a, path_b, False, True)], stats=stats)[0]
    print(kind, got.ssim, stats)
    assert got.ssim >= 0.9 and got.is_duplicate and stats["crop_launches"] == 1
    if kind == "white margins":                                         # the whole file would not have passed
        assert not refine.refine_pairs([(1, 2, path_a, path_b)])[0].is_duplicate


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from PIL import Image

    folder = tmp_path_factory.mktemp("trimmed_ssim_files")
    records = S.write_corpus(folder)
    opened = [np.asarray(Image.open(r["path"]).convert("RGB")) for r in records]
    assert max(max(px.shape[:2]) for px in opened) <= 260
    stored, _, ok = K.hash_batch(opened, want_dhash=False)
    assert ok.all()
    files = [DuplicateFile(r["file_id"], Path(r["path"]), os.path.getsize(r["path"]), px.shape[1], px.shape[0], int(h))
             for r, px, h in zip(records, opened, stored)]
    baseline = api.find_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD)
    return dict(folder=folder, records=records, opened=opened, files=files, baseline=baseline)


def _groups(clusters):
    return {frozenset(e.file.file_id for e in c.files) for c in clusters}


def _facts(m):
    return (m.file_id_a, m.file_id_b, m.trimmed_a, m.trimmed_b, m.hamming, m.box_a, m.box_b)


def test_without_a_threshold_every_decoy_is_linked_and_with_one_none_is(corpus):
    records, files, opened = corpus["records"], corpus["files"], corpus["opened"]
    decoys = {r["file_id"] for r in records if r["decoy"]}
    families = S.families(records)
    base_clusters, base_matches = corpus["baseline"]
    assert len(decoys) == 4 and all(m.ssim is None for m in base_matches)
    # what this route gave before it could look at the pixels: the trimmed pHash links every decoy to its original
    original = {r["original"]: r["file_id"] for r in records if r["kind"] is None}
    base_pairs = {(m.file_id_a, m.file_id_b) for m in base_matches}
    for r in records:
        if r["kind"] is not None and r["original"] != "drawing":
            assert (original[r["original"]], r["file_id"]) in base_pairs, r
    assert all(any(g & decoys for g in _groups(base_clusters) if original[i] in g) for i in S.DECOYS)

    clusters, matches = api.find_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD, ssim_threshold=S.SSIM_THRESHOLD)
    assert _groups(clusters) == families
    pairs = {(m.file_id_a, m.file_id_b) for m in matches}
    assert not any({a, b} & decoys for a, b in pairs)
    for r in records:                                                   # every true copy is still linked to its original, on its box
        if r["kind"] is not None and r["original"] != "drawing" and not r["decoy"]:
            assert (original[r["original"]], r["file_id"]) in pairs, r
    base_facts = {(m.file_id_a, m.file_id_b): _facts(m) for m in base_matches}
    for m in matches:
        assert _facts(m) == base_facts[(m.file_id_a, m.file_id_b)]
        sides = [T.crop(opened[f - 1], T.content_box(opened[f - 1], T.TOLERANCE)) if cut else opened[f - 1]
                 for f, cut in ((m.file_id_a, m.trimmed_a), (m.file_id_b, m.trimmed_b))]
        want = O.ssim_fit(*sides)
        print(m, want)
        assert m.ssim >= S.SSIM_THRESHOLD and abs(m.ssim - want) <= 1e-5, m

    everything, all_matches = api.find_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD, ssim_threshold=0.0)
    assert [_facts(m) for m in all_matches] == [_facts(m) for m in base_matches]
    assert all(m.ssim is not None for m in all_matches) and _groups(everything) == _groups(base_clusters)
    decoy_of = {original[r["original"]]: r["file_id"] for r in records if r["decoy"]}
    scored = {(m.file_id_a, m.file_id_b): m.ssim for m in all_matches}
    assert all(scored[pair] < 0.5 for pair in decoy_of.items())      # the oracle's figure for a decoy's box against its original
    again = api.find_trimmed_duplicates(files, hamming_threshold=T.THRESHOLD, ssim_threshold=None)
    assert again[1] == base_matches and _groups(again[0]) == _groups(base_clusters)


def test_scan_dups_trimmed_ssim_prints_the_same_groups(corpus, tmp_path, capsys):
    files, families = corpus["files"], S.families(corpus["records"])
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
    assert cli.main(["scan-dups", "--db", db, "--trimmed", "--trimmed-ssim", str(S.SSIM_THRESHOLD), "--csv", out_csv]) == 0
    assert f"{len(families)} duplicate group(s), {sum(map(len, families))} file(s)" in capsys.readouterr().out
    with open(out_csv, newline="") as handle:
        table = list(csv.DictReader(handle))
    assert list(table[0]) == cli.CSV_HEADER + ["box"]
    groups: dict = {}
    for row in table:
        groups.setdefault(row["group"], set()).add(int(row["file_id"]))
    assert {frozenset(g) for g in groups.values()} == families
