"""ke_webpa_decode on the GPU: lossy WebP files with an alpha plane against Pillow, bit for bit -- every case family in mixed
batches with the refusals interleaved; the hashes against the oracle's of Pillow's pixels; damaged files refused or equal to
Pillow; a frame near the pixel cap; sub-batches; the batch hasher and the refine seams with KE_GPU_WEBP_ALPHA set and unset."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest
from PIL import Image

import _webp_cases as W
import _webpa_cases as A
import _webpl_cases as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _native():
    from kobato_eyes_amd import _native

    return _native


@pytest.fixture(scope="module")
def ctx():
    return _native().get_context(0)


def test_webpa_decode_matches_pillow_in_mixed_batches(ctx):
    """Families 1-3 and 5 with the refusals (family 4) interleaved, one refused file after every seven taken ones."""
    taken = A.all_taken(A.load_libwebp())
    refused = A.refused_cases()
    batch, expect = [], []
    for k, (family, name, data) in enumerate(taken):
        batch.append(data)
        expect.append((f"{family}:{name}", A.OK))
        if k % 7 == 6:
            name, data, status = refused[(k // 7) % len(refused)]
            batch.append(data)
            expect.append((name, status))
    for name, data, status in refused:                              # and each of them once more at the end
        batch.append(data)
        expect.append((name, status))
    out, status = ctx.webpa_decode(batch)
    families = set()
    for data, px, st, (name, want) in zip(batch, out, status, expect):
        assert st == want, (name, st)
        if want != A.OK:
            assert px is None, name
            continue
        ref = A.pillow_pixels(data)
        assert px.shape == ref.shape and ref.shape[2] == 4, (name, px.shape, ref.shape)
        assert np.array_equal(px, ref), name
        families.add(name[0])
    assert families >= {"1", "3", "5"} and len(taken) > 300


def test_webpa_probe_and_caveats(ctx):
    cases = A.container_cases() + A.raw_cases()[:8]
    w, h, c, st = ctx.webpa_probe([d for _, d, _ in cases])
    for k, (name, data, _) in enumerate(cases):
        assert st[k] == 0 and (h[k], w[k], c[k]) == A.pillow_pixels(data).shape, name


def test_webpa_hash_equals_the_oracle_of_pillow_pixels(ctx):
    cases = [(n, d) for _, n, d in A.all_taken(A.load_libwebp()) if min(A.pillow_pixels(d).shape[:2]) >= 8]
    ph, dh, st = ctx.webpa_hash([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(A.pillow_pixels(data)), name
    assert len(cases) > 150


def test_webpa_damage_is_refused_or_equal_to_pillow(ctx):
    """A bounded sample of the CPU test's damage through the kernels, with its two rules: Pillow still decodes at least a
    quarter of the files, and the decoder takes at least three quarters of those (the CPU build's first run: 92 %)."""
    rng = np.random.default_rng(78)
    damaged = [m for b in A.fuzz_bases() for m in A.damaged(b, rng, 40)]
    out, status = ctx.webpa_decode(damaged)
    decoded = pillow_ok = 0
    for k, (data, px, st) in enumerate(zip(damaged, out, status)):
        assert st in (A.OK, A.UNSUPPORTED, A.CORRUPT)
        ref = A.pillow_pixels(data)
        pillow_ok += ref is not None
        if st == A.OK:
            decoded += 1
            assert ref is not None and px.shape == ref.shape and np.array_equal(ref, px), k
    print(f"damage on the GPU: {len(damaged)} mutations, Pillow decodes {pillow_ok}, the decoder takes {decoded}")
    assert len(damaged) >= 900 and 4 * pillow_ok >= len(damaged) and 4 * decoded >= 3 * pillow_ok


def _big_cases():
    rng = np.random.default_rng(12)
    w, h = 4096, 4080                                                # 256 x 255 macroblocks: 65 280 of the cap's 65 536
    rgb = W.content(rng, w, h, "smooth")
    near_cap = A.pillow_file(rgb, A.plane(rng, w, h, "disc"), 60, 0, 100)
    tall = A.mux(A.frame(rng, 300, 1400), A.raw_alph(A.plane(rng, 300, 1400, "smooth"), 3))     # more rows in a step than the workgroup has lanes
    wide = A.pillow_file(W.content(rng, 1900, 700, "drawing"), A.plane(rng, 1900, 700, "smooth"), 70, 4, 100)
    return [("near_cap", near_cap), ("tall_gradient", tall), ("wide_smooth", wide)] + A.pillow_cases(seed=13, n=24)


def test_a_frame_near_the_pixel_cap_and_many_sub_batches(ctx, monkeypatch):
    """A 4096 x 4080 file beside smaller ones; whole, and cut into sub-batches by a 1 MiB scratch budget: the same pixels as
    Pillow either way."""
    cases = _big_cases()
    refs = [A.pillow_pixels(d) for _, d in cases]
    out, status = ctx.webpa_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, out, status, refs):
        assert st == A.OK and px.shape == ref.shape and np.array_equal(px, ref), name
    monkeypatch.setenv("KE_WEBP_SCRATCH_BYTES", str(1 << 20))
    again, status = ctx.webpa_decode([d for _, d in cases])
    for (name, _), px, st, ref in zip(cases, again, status, refs):
        assert st == A.OK and px.shape == ref.shape and np.array_equal(px, ref), name


def _write(tmp_path, cases, first=0):
    items = []
    for k, (_, data) in enumerate(cases):
        p = tmp_path / f"{first + k:03d}.webp"
        p.write_bytes(data)
        items.append((900 + first + k, str(p)))
    return items


def test_batch_hasher_rows_with_the_alpha_route_on_and_off(tmp_path, monkeypatch):
    """Plain lossy, lossy + alpha and lossless files in the same .webp batch: the Pillow route's rows with KE_GPU_WEBP_ALPHA=1
    as without it, and the alpha files reach the Pillow share only when it is unset."""
    from kobato_eyes_amd import fastsig as K

    lossy = [c for c in W.taken_cases() if min(W.pillow_rgb(c[1]).shape[:2]) >= 8][:30]
    alpha = [(n, d) for _, n, d in A.all_taken(None) if min(A.pillow_pixels(d).shape[:2]) >= 8][:60]
    lossless = [c for c in L.taken_cases() if min(L.pillow_pixels(c[1]).shape[:2]) >= 8][:20]
    others = [(n, d) for n, d, _ in A.refused_cases() if n in ("animated", "alph_without_flag")]       # Pillow's either way
    items = _write(tmp_path, lossy + alpha + lossless + others)
    seen = []
    original = K._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        seen.extend(self.paths[k] for k in todo)
        return original(self, todo, out)

    monkeypatch.setattr(K._Pipeline, "_decode_with_pillow", spy)
    fill = lambda todo: K.fast_fill_missing_signatures("", todo, max_workers=4, chunksize=16, apply_to_db=False)      # noqa: E731
    monkeypatch.delenv("KE_GPU_WEBP_LOSSLESS", raising=False)
    monkeypatch.delenv("KE_GPU_WEBP_ALPHA", raising=False)
    monkeypatch.setenv("KE_GPU_WEBP", "0")                                   # every file through Pillow: the rows to equal
    want = fill(items)
    assert len(want) == len(items)
    monkeypatch.delenv("KE_GPU_WEBP")
    alpha_paths = {p for _, p in items[len(lossy): len(lossy) + len(alpha)]}
    lossless_paths = {p for _, p in items[len(lossy) + len(alpha): len(lossy) + len(alpha) + len(lossless)]}
    other_paths = {p for _, p in items[len(lossy) + len(alpha) + len(lossless):]}
    seen.clear()
    assert fill(items) == want
    assert alpha_paths | lossless_paths | other_paths <= set(seen)           # the variable unset: as before
    monkeypatch.setenv("KE_GPU_WEBP_ALPHA", "1")
    seen.clear()
    assert fill(items) == want
    assert not alpha_paths & set(seen), "a file with an alpha plane went to the Pillow share"
    assert lossless_paths | other_paths <= set(seen)                         # independent of KE_GPU_WEBP_LOSSLESS
    monkeypatch.setenv("KE_GPU_WEBP_LOSSLESS", "1")
    seen.clear()
    assert fill(items) == want
    assert not (alpha_paths | lossless_paths) & set(seen) and other_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_WEBP", "0")                                   # the whole WebP route off: the variables alone do nothing
    seen.clear()
    assert fill(items) == want
    assert alpha_paths <= set(seen)


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


def _refine_files(tmp_path):
    """Eight near-duplicates with alpha planes (two of them carrying an EXIF orientation) and one plain lossy file"""
    rng = np.random.default_rng(3)
    base = O.synth_rgb(4242, 96, 80)
    files = []
    for k in range(8):
        px = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) if k % 2 else base
        alpha = A.plane(rng, 96, 80, A.ALPHA_KINDS[k % 5])
        data = A.pillow_file(px, alpha, 70 + k, 4, (100, 60)[k % 2])
        if k in (2, 5):
            data = A.mux(A.vp8_of(data), A.alph_of(data), 0x18, after=[(b"EXIF", A.exif_blob(6))])
        p = tmp_path / f"a{k}.webp"
        p.write_bytes(data)
        files.append(p)
    plain = tmp_path / "a8.webp"
    plain.write_bytes(W.pillow_file(base, 80, 4))
    files.append(plain)
    return files


def test_refine_pairs_with_the_alpha_route_on_and_off(tmp_path, monkeypatch):
    import kobato_eyes_amd as KA

    files = _refine_files(tmp_path)
    pairs = [(a, b, files[a], files[b]) for a, b in [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 5), (3, 7), (8, 1), (8, 2)]]
    th = KA.RefinementThresholds(ssim=0.9)
    monkeypatch.delenv("KE_GPU_WEBP_ALPHA", raising=False)
    monkeypatch.setenv("KE_GPU_REFINE_DECODE", "0")                          # the loader route: the values to equal, to the last bit
    want = KA.refine_pairs(pairs, thresholds=th)
    assert all(m is not None and m.ssim is not None for m in want)
    monkeypatch.delenv("KE_GPU_REFINE_DECODE")
    stats = {}
    assert KA.refine_pairs(pairs, thresholds=th, stats=stats) == want
    assert stats["gpu_decodes"] == 1 and "gpu_normalised" not in stats, stats           # the plain lossy file alone
    monkeypatch.setenv("KE_GPU_WEBP_ALPHA", "1")
    stats = {}
    assert KA.refine_pairs(pairs, thresholds=th, stats=stats) == want
    assert stats["gpu_normalised"] == 6 and stats["gpu_decodes"] == 7, stats            # EXIF: the loader decides


def test_refine_parallel_stages_with_the_alpha_route_on_and_off(tmp_path, monkeypatch):
    import kobato_eyes_amd as KA
    from kobato_eyes_amd import refine_parallel as RP

    files = _refine_files(tmp_path)
    clusters = [Cl([E(F(k, files[k])) for k in (0, 1, 2, 3, 8)], 0), Cl([E(F(k, files[k])) for k in range(4, 8)], 4)]
    ids = lambda found: [[c.keeper_id, [e.file.file_id for e in c.files]] for c in found]      # noqa: E731
    monkeypatch.delenv("KE_GPU_WEBP_ALPHA", raising=False)
    assert set(RP._thumbnails_decoded_on_gpu(files, 32, 0)) == {files[8]}
    want_tiles = ids(KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2))
    want_pixels = ids(KA.refine_by_pixels_parallel(clusters, mae_thr=0.05, thumb_size=64, workers=2))
    assert want_tiles and want_pixels
    monkeypatch.setenv("KE_GPU_WEBP_ALPHA", "1")
    for side in (32, 64):
        on_gpu = RP._thumbnails_decoded_on_gpu(files, side, 0)
        assert set(on_gpu) == {p for k, p in enumerate(files) if k not in (2, 5)}      # EXIF: the loader decides
        for p, t in on_gpu.items():
            assert np.array_equal(t, RP._thumbnails([RP._decode(p)], side, 0)[0]), p
    assert ids(KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)) == want_tiles
    assert ids(KA.refine_by_pixels_parallel(clusters, mae_thr=0.05, thumb_size=64, workers=2)) == want_pixels
    # the MAE values themselves: the GPU route's thumbnails give the loader route's sums
    ctx = _native().get_context(0)
    thumbs = np.stack([RP._thumbnails_decoded_on_gpu(files, 64, 0)[files[k]] for k in (0, 1, 3, 4)])
    loader = np.stack(RP._thumbnails([RP._decode(files[k]) for k in (0, 1, 3, 4)], 64, 0))
    sad = lambda t: ctx.sad_pairs(t.reshape(4, -1), 4, 64 * 64, [1, 2, 3], [0, 0, 0]).tolist()      # noqa: E731
    assert sad(thumbs) == sad(loader)
