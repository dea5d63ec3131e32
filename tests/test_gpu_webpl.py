"""ke_webpl_decode on the GPU: lossless WebP files (one VP8L bitstream) against Pillow, bit for bit -- shape, channels and
pixels -- in one mixed batch with the test writer's files and the refusals; the hashes against the oracle's of Pillow's
pixels; damaged files refused or equal to Pillow; large frames whole and in sub-batches; the batch hasher and the refine seams
with KE_GPU_WEBP_LOSSLESS set and unset."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest
from PIL import Image

import _vp8l_write as V
import _webp_cases as W
import _webpl_cases as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _native():
    from kobato_eyes_amd import _native

    return _native


@pytest.fixture(scope="module")
def ctx():
    return _native().get_context(0)


def test_webpl_decode_matches_pillow_in_one_mixed_batch(ctx):
    cases = L.taken_cases() + [(n, d) for n, d, _ in V.written_cases()]
    refused = L.refused_cases()
    out, status = ctx.webpl_decode([d for _, d in cases] + [d for _, d, _ in refused])
    channels = set()
    for k, (name, data) in enumerate(cases):
        assert status[k] == L.OK, name
        ref = L.pillow_pixels(data)
        assert out[k].shape == ref.shape, (name, out[k].shape, ref.shape)
        assert np.array_equal(out[k], ref), name
        channels.add(ref.shape[2])
    for k, (name, _, expected) in enumerate(refused, len(cases)):
        assert status[k] == expected and out[k] is None, name
    assert len(cases) > 250 and channels == {3, 4}


def test_webpl_probe_reports_what_pillow_opens(ctx):
    cases = L.wrapped_cases() + L.palette_cases()
    w, h, c, st = ctx.webpl_probe([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        assert st[k] == 0 and (h[k], w[k], c[k]) == L.pillow_pixels(data).shape, name


def test_webpl_hash_equals_the_oracle_of_pillow_pixels(ctx):
    cases = [(n, d) for n, d in L.taken_cases() if min(L.pillow_pixels(d).shape[:2]) >= 8]
    ph, dh, st = ctx.webpl_hash([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(L.pillow_pixels(data)), name
    assert len(cases) > 100


def test_webpl_damage_is_refused_or_equal_to_pillow(ctx):
    rng = np.random.default_rng(77)
    damaged = [m for b in L.fuzz_bases() for m in L.damaged(b, rng, 40)]
    out, status = ctx.webpl_decode(damaged)
    decoded = 0
    for k, (data, px, st) in enumerate(zip(damaged, out, status)):
        assert st in (L.OK, L.UNSUPPORTED, L.CORRUPT)
        if st == L.OK:
            decoded += 1
            ref = L.pillow_pixels(data)
            assert ref is not None and px.shape == ref.shape and np.array_equal(ref, px), k
    assert len(damaged) >= 500 and decoded > 25


def test_large_frames_and_many_sub_batches(ctx, monkeypatch):
    """A ~2 000 x 1 300 drawing and a textured frame (more rows in a wavefront step than the workgroup has lanes), beside
    smaller files; whole, and cut into sub-batches by a 1 MiB scratch budget: the same pixels as Pillow either way."""
    rng = np.random.default_rng(12)
    textured = (W.content(rng, 1900, 1250, "smooth").astype(np.int16) + rng.integers(-6, 7, (1250, 1900, 3))).clip(0, 255).astype(np.uint8)
    big = [("big_drawing", L.pillow_file(Image.fromarray(W.content(rng, 2000, 1300, "drawing")), 75, 4)),
           ("big_textured", L.pillow_file(Image.fromarray(textured), 40, 2))]
    cases = big + L.pillow_cases(seed=13, n=24)
    refs = [L.pillow_pixels(d) for _, d in cases]
    out, status = ctx.webpl_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, out, status, refs):
        assert st == L.OK and px.shape == ref.shape and np.array_equal(px, ref), name
    monkeypatch.setenv("KE_WEBP_SCRATCH_BYTES", str(1 << 20))
    out, status = ctx.webpl_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, out, status, refs):
        assert st == L.OK and px.shape == ref.shape and np.array_equal(px, ref), name


def _write(tmp_path, cases, first=0):
    items = []
    for k, (_, data) in enumerate(cases):
        p = tmp_path / f"{first + k:03d}.webp"
        p.write_bytes(data)
        items.append((900 + first + k, str(p)))
    return items


def test_batch_hasher_rows_with_the_lossless_route_on_and_off(tmp_path, monkeypatch):
    """Lossy and lossless files in the same .webp batch: the same rows with KE_GPU_WEBP_LOSSLESS=1 as without it, and the
    lossless files reach the Pillow share only when it is unset."""
    from kobato_eyes_amd import fastsig as K

    lossy = [c for c in W.taken_cases() if min(W.pillow_rgb(c[1]).shape[:2]) >= 8][:30]
    lossless = [c for c in L.taken_cases() if min(L.pillow_pixels(c[1]).shape[:2]) >= 8][:50]
    others = [(n, d) for n, d, _ in L.refused_cases()[1:3]]                   # lossy + ALPH, animated: Pillow's either way
    items = _write(tmp_path, lossy + lossless + others)
    seen = []
    original = K._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        seen.extend(self.paths[k] for k in todo)
        return original(self, todo, out)

    monkeypatch.setattr(K._Pipeline, "_decode_with_pillow", spy)
    monkeypatch.delenv("KE_GPU_WEBP_LOSSLESS", raising=False)
    rows = K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    lossless_paths = {p for _, p in items[len(lossy): len(lossy) + len(lossless)]}
    other_paths = {p for _, p in items[len(lossy) + len(lossless):]}
    assert lossless_paths | other_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_WEBP_LOSSLESS", "1")
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16) and len(rows) == len(items)
    assert not lossless_paths & set(seen), "a lossless file went to the Pillow share"
    assert other_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_WEBP", "0")                                   # the whole WebP route off: the variable alone does nothing
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert lossless_paths <= set(seen)


def test_refine_seams_with_the_lossless_route_on_and_off(tmp_path, monkeypatch):
    import kobato_eyes_amd as KA
    from kobato_eyes_amd import refine_parallel as RP

    rng = np.random.default_rng(3)
    base = O.synth_rgb(4242, 96, 80)
    files = []
    for k in range(8):
        px = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) if k % 2 else base
        body = L.vp8l_of(L.pillow_file(Image.fromarray(px), 70 + k, 4))
        data = L.vp8x(body, 0x08, after=[(b"EXIF", L.exif_blob(6))]) if k in (2, 5) else L.riff([(b"VP8L", body)])
        p = tmp_path / f"w{k}.webp"
        p.write_bytes(data)
        files.append(p)
    rgba = tmp_path / "w8.webp"                                  # an RGBA file stays with the loader
    rgba.write_bytes(L.pillow_file(L._rgba(rng, base)))
    files.append(rgba)
    monkeypatch.delenv("KE_GPU_WEBP_LOSSLESS", raising=False)
    assert RP._thumbnails_decoded_on_gpu(files, 32, 0) == {}

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
    want_pairs = KA.refine_pairs(pairs, thresholds=th, stats=stats)
    want_tiles = [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)]
    assert stats["gpu_decodes"] == 0, stats
    monkeypatch.setenv("KE_GPU_WEBP_LOSSLESS", "1")
    on_gpu = RP._thumbnails_decoded_on_gpu(files, 32, 0)
    assert set(on_gpu) == {p for k, p in enumerate(files) if k not in (2, 5, 8)}    # EXIF, RGBA: the loader decides
    for p, t in on_gpu.items():
        assert np.array_equal(t, RP._thumbnails([RP._decode(p)], 32, 0)[0]), p
    stats = {}
    assert KA.refine_pairs(pairs, thresholds=th, stats=stats) == want_pairs and stats["gpu_decodes"] == 6, stats
    assert [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)] == want_tiles
