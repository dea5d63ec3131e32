"""ke_webp_decode on the GPU: lossy WebP files (one VP8 key frame) against Pillow, pixel for pixel, in one mixed batch with the
refusals; the hashes against the oracle's of Pillow's pixels; damaged files refused or equal to Pillow; the batch hasher and
the refine seams with the route on and off."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import pytest

import _vp8_rewrite as R
import _webp_cases as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _native():
    from kobato_eyes_amd import _native

    return _native


@pytest.fixture(scope="module")
def ctx():
    return _native().get_context(0)


def test_webp_decode_matches_pillow_in_one_mixed_batch(ctx):
    cases = W.taken_cases()
    refused = W.refused_cases()
    out, status = ctx.webp_decode([d for _, d in cases] + [d for _, d, _ in refused])
    for k, (name, data) in enumerate(cases):
        assert status[k] == W.OK, name
        ref = W.pillow_rgb(data)
        assert out[k].shape == ref.shape and np.array_equal(out[k], ref), name
    for k, (name, _, expected) in enumerate(refused, len(cases)):
        assert status[k] == expected and out[k] is None, name
    assert len(cases) > 200


def test_webp_hash_equals_the_oracle_of_pillow_pixels(ctx):
    cases = [(n, d) for n, d in W.taken_cases() if min(W.pillow_rgb(d).shape[:2]) >= 8]
    ph, dh, st = ctx.webp_hash([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(W.pillow_rgb(data)), name


def test_webp_damage_is_refused_or_equal_to_pillow(ctx):
    rng = np.random.default_rng(77)
    bases = [d for _, d in W.pillow_cases(seed=9, n=12)] + [d for _, d in W.golden_cases()[:8]]
    damaged = [m for b in bases for m in W.damaged(b, rng, 30)]
    out, status = ctx.webp_decode(damaged)
    decoded = 0
    for k, (data, px, st) in enumerate(zip(damaged, out, status)):
        assert st in (W.OK, W.UNSUPPORTED, W.CORRUPT)
        if st == W.OK:
            decoded += 1
            ref = W.pillow_rgb(data)
            assert ref is not None and np.array_equal(ref, px), k
    assert len(damaged) >= 500 and decoded > 50


def _write(tmp_path, cases, first=0):
    items = []
    for k, (_, data) in enumerate(cases):
        p = tmp_path / f"{first + k:03d}.webp"
        p.write_bytes(data)
        items.append((900 + first + k, str(p)))
    return items


def test_batch_hasher_rows_with_the_route_on_and_off(tmp_path, monkeypatch):
    from kobato_eyes_amd import fastsig as K

    lossy = [c for c in W.taken_cases() if min(W.pillow_rgb(c[1]).shape[:2]) >= 8][:60]
    others = [(n, d) for n, d, _ in W.refused_cases()[:3]]                    # lossless, alpha, animated: Pillow's
    up = [(n, d) for n, d, _ in R.quant_up_cases()]                           # over the coefficient limit: Pillow's
    _, status = _native().get_context(0).webp_decode([d for _, d in up])
    others += [c for c, st in zip(up, status) if st == W.UNSUPPORTED]
    assert len(others) >= 3 + 10
    items = _write(tmp_path, lossy + others)
    seen = []
    original = K._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        seen.extend(self.paths[k] for k in todo)
        return original(self, todo, out)

    monkeypatch.setattr(K._Pipeline, "_decode_with_pillow", spy)
    rows = K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    lossy_paths = {p for _, p in items[: len(lossy)]}
    assert not lossy_paths & set(seen), "a lossy file went to the Pillow share"
    assert {p for _, p in items[len(lossy):]} <= set(seen)
    monkeypatch.setenv("KE_GPU_WEBP", "0")
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16) and len(rows) == len(items)
    assert lossy_paths <= set(seen)


def test_refine_seams_with_the_route_on_and_off(tmp_path, monkeypatch):
    import kobato_eyes_amd as KA
    from kobato_eyes_amd import refine_parallel as RP

    rng = np.random.default_rng(3)
    base = O.synth_rgb(4242, 96, 80)
    files = []
    for k in range(8):
        px = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) if k % 2 else base
        vp8 = W.vp8_of(W.pillow_file(px, 70 + k, 4))
        data = W.vp8x(vp8, 0x08, after=[(b"EXIF", W.exif_blob(6))]) if k in (2, 5) else W.riff([(b"VP8 ", vp8)])
        p = tmp_path / f"w{k}.webp"
        p.write_bytes(data)
        files.append(p)
    turned = tmp_path / "w8.webp"                                # an orientation in XMP only: exif_transpose turns it too
    turned.write_bytes(W.xmp_turned_file())
    files.append(turned)
    on_gpu = RP._thumbnails_decoded_on_gpu(files, 32, 0)
    assert set(on_gpu) == {p for k, p in enumerate(files) if k not in (2, 5, 8)}    # EXIF / XMP: the loader decides
    for p, t in on_gpu.items():
        assert np.array_equal(t, RP._thumbnails([RP._decode(p)], 32, 0)[0]), p

    @dataclass
    class F:
        file_id: int
        path: object

    @dataclass
    class E:
        file: F

    @dataclass
    class Cl:
        files: list
        keeper_id: int

    clusters = [Cl([E(F(k, files[k])) for k in (0, 1, 2, 3, 8)], 0), Cl([E(F(k, files[k])) for k in range(4, 8)], 4)]
    pairs = [(a, b, files[a], files[b]) for a, b in [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 5), (3, 7), (8, 1), (8, 2)]]
    th = KA.RefinementThresholds(ssim=0.9)
    stats = {}
    got_pairs = KA.refine_pairs(pairs, thresholds=th, stats=stats)
    got_tiles = [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)]
    assert stats["gpu_decodes"] == 6, stats
    monkeypatch.setenv("KE_GPU_WEBP", "0")
    stats = {}
    assert KA.refine_pairs(pairs, thresholds=th, stats=stats) == got_pairs and stats["gpu_decodes"] == 0
    assert [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)] == got_tiles
    assert RP._thumbnails_decoded_on_gpu(files, 32, 0) == {}


def test_large_frames_and_many_sub_batches(ctx, monkeypatch):
    """A frame whose wavefront steps hold more macroblocks than a wave has lanes (2 176 x 1 088: 68 in one step), and a batch
    cut into many sub-batches by a small scratch budget: the same pixels as Pillow either way."""
    rng = np.random.default_rng(12)
    big = [("big_smooth", W.pillow_file(W.content(rng, 2176, 1088, "smooth"), 60, 2)),
           ("big_drawing", W.pillow_file(W.content(rng, 2100, 1300, "drawing"), 85, 4))]
    cases = big + [(n, d) for n, d in W.pillow_cases(seed=13, n=24)]
    refs = [W.pillow_rgb(d) for _, d in cases]
    out, status = ctx.webp_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, out, status, refs):
        assert st == W.OK and np.array_equal(px, ref), name
    monkeypatch.setenv("KE_WEBP_SCRATCH_BYTES", str(1 << 20))           # about one 512 x 512 frame per sub-batch
    out, status = ctx.webp_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, out, status, refs):
        assert st == W.OK and np.array_equal(px, ref), name


# ---- rewritten key frames (tests/_vp8_rewrite.py): header fields and modes no encoder writes ----------------------------------
@pytest.fixture(scope="module")
def rewritten():
    return {g: [(n, d) for n, d, _ in fn()] for g, fn in R.GROUPS.items()}


def test_rewritten_files_match_pillow_in_one_mixed_batch(ctx, rewritten):
    """All five groups with the taken and refused cases in one call.  modes / filter / header / quant_down: pixel-equal to
    Pillow, no exemptions; quant_up: equal to Pillow or refused (the coefficient limit) where Pillow decodes, at least 10
    of each; nothing Pillow refuses comes back OK."""
    groups = [(g, n, d) for g, cases in rewritten.items() for n, d in cases]
    taken, refused = W.taken_cases(), W.refused_cases()
    blobs = [d for _, _, d in groups] + [d for _, d in taken] + [d for _, d, _ in refused]
    out, status = ctx.webp_decode(blobs)
    split = {W.OK: 0, W.UNSUPPORTED: 0}
    for k, (group, name, data) in enumerate(groups):
        ref = W.pillow_rgb(data)
        if ref is None:
            assert status[k] != W.OK, f"{name}: decoded where Pillow refuses"
            continue
        if group == "quant_up" and status[k] == W.UNSUPPORTED:
            assert out[k] is None, name
        else:
            assert status[k] == W.OK, name
            assert out[k].shape == ref.shape and np.array_equal(out[k], ref), name
        if group == "quant_up":
            split[int(status[k])] += 1
    print(f"quant_up: {split[W.OK]} taken, {split[W.UNSUPPORTED]} refused")
    assert split[W.OK] >= 10 and split[W.UNSUPPORTED] >= 10
    for k, (name, data) in enumerate(taken, len(groups)):
        assert status[k] == W.OK and np.array_equal(out[k], W.pillow_rgb(data)), name
    for k, (name, _, expected) in enumerate(refused, len(groups) + len(taken)):
        assert status[k] == expected and out[k] is None, name


def test_rewritten_hashes_equal_the_oracle_of_pillow_pixels(ctx, rewritten):
    cases = [(n, d) for g, cs in rewritten.items() for n, d in cs if min(W.pillow_rgb(d).shape[:2]) >= 8]
    ph, dh, st = ctx.webp_hash([d for _, d in cases])
    hashed = 0
    for k, (name, data) in enumerate(cases):
        if name.startswith("qup_") and st[k] == W.UNSUPPORTED:
            continue
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(W.pillow_rgb(data)), name
        hashed += 1
    assert hashed >= 300


def test_large_rewritten_frame_whole_and_in_sub_batches(ctx, rewritten, monkeypatch):
    """2 176 x 1 088 with random modes and the strongest normal filter: 68 macroblocks in a wavefront step, beside the
    rewritten files of the filter group; whole and cut into sub-batches by a 1 MiB scratch budget."""
    cases = [R.big_frame_case()] + rewritten["filter"][:24]
    refs = [W.pillow_rgb(d) for _, d in cases]
    out, status = ctx.webp_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, out, status, refs):
        assert st == W.OK and np.array_equal(px, ref), name
    monkeypatch.setenv("KE_WEBP_SCRATCH_BYTES", str(1 << 20))
    out, status = ctx.webp_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, out, status, refs):
        assert st == W.OK and np.array_equal(px, ref), name
