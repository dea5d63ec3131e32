"""ke_tiffc_decode on the GPU: LZW and PackBits TIFF files against Pillow / libtiff, bit for bit -- shape, channels and pixels --
in one shuffled batch with the refusals; damaged files refused or equal to Pillow; sub-batches; a batch mixing compressed and
uncompressed files; a file near the pixel cap; the batch hasher and the refine seams with KE_GPU_TIFF_COMPRESSED set and
unset.  Every call is one bounded batch of small files (the large ones are flat and walk in a few thousand codes)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest
from PIL import Image

import _tiff_cases as T
import _tiffc_cases as A
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _native():
    from kobato_eyes_amd import _native

    return _native


@pytest.fixture(scope="module")
def ctx():
    return _native().get_context(0)


def _check(cases, out, status):
    for (name, data), px, st in zip(cases, out, status):
        ref = A.pillow_pixels(data)
        assert st == A.OK, (name, st)
        assert px.shape == ref.shape, (name, px.shape, ref.shape)
        assert np.array_equal(px, ref), name


def test_every_valid_file_equals_pillow_in_one_shuffled_batch(ctx):
    cases = [(n, d) for _, n, d in A.valid_cases()]
    refused = A.refused_cases()
    everything = [(n, d, A.OK) for n, d in cases] + refused
    order = np.random.default_rng(7).permutation(len(everything))
    out, status = ctx.tiffc_decode([everything[k][1] for k in order])
    shapes = set()
    for k, px, st in zip(order.tolist(), out, status):
        name, data, expected = everything[k]
        assert st == expected, (name, st)
        if expected != A.OK:
            assert px is None, name
            continue
        ref = A.pillow_pixels(data)
        assert px.shape == ref.shape, (name, px.shape, ref.shape)
        assert np.array_equal(px, ref), name
        shapes.add(ref.shape[2] if ref.ndim == 3 else 1)
    assert len(cases) > 300 and shapes == {1, 3, 4}


def test_the_copy_patterns_of_the_gif_streams_equal_pillow(ctx):
    """The shared sink (csrc/ke_lz_records.h) and the copies at length bias 2 on this consumer: runs of every distance 2..17, at
    the start of the records and across a round of 64, and last strings cut to one byte, in one call with a time limit of
    its own (a call that hangs in native code ends the run: nothing more is started on the device)."""
    import faulthandler

    cases = A.sink_cases()
    faulthandler.dump_traceback_later(60, exit=True)
    try:
        out, status = ctx.tiffc_decode([d for _, d in cases])
    finally:
        faulthandler.cancel_dump_traceback_later()
    _check(cases, out, status)
    assert len(cases) >= 100


def test_probe_reports_what_pillow_opens(ctx):
    cases = A.pillow_cases()[::3] + A.handmade_cases()[::5]
    w, h, c, st = ctx.tiffc_probe([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        ref = A.pillow_pixels(data)
        assert st[k] == 0 and (h[k], w[k]) == ref.shape[:2] and c[k] == (ref.shape[2] if ref.ndim == 3 else 1), name


def test_hash_equals_the_oracle_of_pillow_pixels(ctx):
    cases = [(n, d) for n, d in A.pillow_cases() if min(A.pillow_pixels(d).shape[:2]) >= 8]
    ph, dh, st = ctx.tiffc_hash([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(A.pillow_pixels(data)), name
    assert len(cases) >= 60


def test_late_change_and_damage_are_refused_or_equal_to_pillow(ctx):
    """The damaged set of tests/test_tiffc_cpu.py -- the same 5 600 files (A.damaged_set) -- and the late-change streams through
    the kernels in one batch: taken => strict Pillow takes it with equal pixels.  The census is printed; the kernels run the
    arithmetic of the CPU build, so it is that test's (LZW: Pillow takes 995 of 2 800, the decoder 940; PackBits: 1 652 and
    1 605), and so are the floors, 20 % under it: 750 and 1 280."""
    late = [(A.LZW, d) for _, d in A.late_change_cases()]
    files = A.damaged_set() + late
    out, status = ctx.tiffc_decode([d for _, d in files])
    census = {c: {"cases": 0, "pillow": 0, "taken": 0} for c in (A.LZW, A.PACKBITS)}
    for k, ((comp, data), px, st) in enumerate(zip(files, out, status)):
        assert st in (A.OK, A.UNSUPPORTED, A.CORRUPT)
        counted = k < len(files) - len(late)
        ref = A.pillow_pixels(data)
        census[comp]["cases"] += counted
        census[comp]["pillow"] += counted and ref is not None
        if st == A.OK:
            census[comp]["taken"] += counted
            assert ref is not None and px.shape == ref.shape and np.array_equal(ref, px), k
    for comp, c in census.items():
        print(f"damage census through the kernels, compression {comp}: {c['cases']} cases, Pillow takes {c['pillow']}, the decoder takes {c['taken']}")
    assert sum(c["cases"] for c in census.values()) >= 5000
    assert census[A.LZW]["taken"] >= 750 and census[A.PACKBITS]["taken"] >= 1280


def test_sub_batches_and_a_batch_with_uncompressed_files(ctx, monkeypatch):
    """The same files whole and cut into sub-batches by a 256 KiB scratch budget; uncompressed files in the batch are refused
    here (status 1: they are ke_tiff_decode's) and taken there, the compressed ones the other way round."""
    cases = A.pillow_cases()[40:] + A.lzw_stream_cases()[:8]
    plain = [(n, d) for n, d, _ in list(T.supported())[:8]]
    mixed = [x for pair in zip(cases, plain * (len(cases) // len(plain) + 1)) for x in pair]
    is_plain = [k % 2 == 1 for k in range(len(mixed))]
    for budget in (None, 1 << 18):
        if budget:
            monkeypatch.setenv("KE_TIFFC_SCRATCH_BYTES", str(budget))
        out, status = ctx.tiffc_decode([d for _, d in mixed])
        _check([c for c, p in zip(mixed, is_plain) if not p], [o for o, p in zip(out, is_plain) if not p], [s for s, p in zip(status, is_plain) if not p])
        assert all(s == A.UNSUPPORTED for s, p in zip(status, is_plain) if p)
    monkeypatch.delenv("KE_TIFFC_SCRATCH_BYTES")
    out, status = ctx.tiff_decode([d for _, d in mixed])
    assert all((s == 0) == p for s, p in zip(status, is_plain))
    for (name, data), px, p in zip(mixed, out, is_plain):
        if p:
            assert np.array_equal(px, T._pillow(data)), name


def test_a_file_near_the_pixel_cap(ctx):
    """8 192 x 8 190 gray (the cap is 2^26 pixels), flat with a few rectangles, as libtiff writes it with LZW (predictor 2) and
    with PackBits -- 1 024 strips of 8 rows; one row more than the cap allows is refused."""
    import io

    def written(a, **how):
        b = io.BytesIO()
        Image.fromarray(a).save(b, "TIFF", **how)
        return b.getvalue()

    a = np.full((8190, 8192), 200, np.uint8)
    a[1000:3000, 500:7000] = 17
    a[5000:5003, :] = 90
    a[:, 4000:4002] = 3
    for how in (dict(compression="tiff_lzw", tiffinfo={317: 2}), dict(compression="packbits")):
        out, status = ctx.tiffc_decode([written(a, **how)])
        assert status[0] == A.OK and np.array_equal(out[0], a), how
    beyond = written(np.zeros((8193, 8192), np.uint8), compression="packbits")
    assert ctx.tiffc_probe([beyond])[3][0] == A.UNSUPPORTED


def _write(tmp_path, cases, first=0):
    items = []
    for k, (_, data) in enumerate(cases):
        p = tmp_path / f"{first + k:03d}.tif"
        p.write_bytes(data)
        items.append((900 + first + k, str(p)))
    return items


def test_batch_hasher_rows_with_the_compressed_route_on_and_off(tmp_path, monkeypatch):
    """Uncompressed, LZW and PackBits files in the same .tif batch: the same rows with KE_GPU_TIFF_COMPRESSED=1 as without it,
    and the compressed files reach the Pillow share only when it is unset."""
    from kobato_eyes_amd import fastsig as K

    big_enough = lambda d: min(A.pillow_pixels(d).shape[:2]) >= 8
    plain = [(n, d) for n, d, _ in T.supported() if big_enough(d)][:12]
    packed = [(n, d) for n, d in A.pillow_cases() + A.lzw_stream_cases()[:6] if big_enough(d)][:60]
    others = [(n, d) for n, d, _ in A.refused_cases() if n in ("deflate", "orientation_6", "lzw_no_opening_clear")]
    items = _write(tmp_path, plain + packed + others)
    seen = []
    original = K._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        seen.extend(self.paths[k] for k in todo)
        return original(self, todo, out)

    monkeypatch.setattr(K._Pipeline, "_decode_with_pillow", spy)
    monkeypatch.delenv("KE_GPU_TIFF_COMPRESSED", raising=False)
    rows = K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    plain_paths = {p for _, p in items[:len(plain)]}
    packed_paths = {p for _, p in items[len(plain): len(plain) + len(packed)]}
    other_paths = {p for _, p in items[len(plain) + len(packed):]}
    assert packed_paths | other_paths <= set(seen) and not plain_paths & set(seen)
    assert len(rows) >= len(plain) + len(packed)                            # (what Pillow itself fails on has no row, either way)
    monkeypatch.setenv("KE_GPU_TIFF_COMPRESSED", "1")
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert not (packed_paths | plain_paths) & set(seen), "a file the GPU decoders take went to the Pillow share"
    assert other_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_TIFF", "0")                                   # the whole TIFF route off: the variable alone does nothing
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert packed_paths | plain_paths <= set(seen)


def test_refine_seams_with_the_compressed_route_on_and_off(tmp_path, monkeypatch):
    import kobato_eyes_amd as KA
    from kobato_eyes_amd import refine_parallel as RP

    rng = np.random.default_rng(3)
    base = O.synth_rgb(4242, 96, 80)
    files = []
    for k in range(8):
        px = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) if k % 2 else base
        if k in (2, 5):                                                  # an orientation to apply: the loader's
            data = A.compressed(px, A.LZW, rows=16, more=[(274, 3, 1, [6])])
        else:
            data = A.pillow_file(np.dstack([px, px[..., :1]]), "RGB", "tiff_lzw" if k % 4 else "packbits", k % 3 == 0)
        p = tmp_path / f"t{k}.tif"
        p.write_bytes(data)
        files.append(p)
    monkeypatch.delenv("KE_GPU_TIFF_COMPRESSED", raising=False)
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

    clusters = [Cl([E(F(k, files[k])) for k in range(4)], 0), Cl([E(F(k, files[k])) for k in range(4, 8)], 4)]
    pairs = [(a, b, files[a], files[b]) for a, b in [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 5), (3, 7)]]
    th = KA.RefinementThresholds(ssim=0.9)
    stats = {}
    want_pairs = KA.refine_pairs(pairs, thresholds=th, stats=stats)
    want_tiles = [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)]
    assert stats["gpu_decodes"] == 0, stats
    monkeypatch.setenv("KE_GPU_TIFF_COMPRESSED", "1")
    on_gpu = RP._thumbnails_decoded_on_gpu(files, 32, 0)
    assert set(on_gpu) == {p for k, p in enumerate(files) if k not in (2, 5)}
    for p, t in on_gpu.items():
        assert np.array_equal(t, RP._thumbnails([RP._decode(p)], 32, 0)[0]), p
    stats = {}
    assert KA.refine_pairs(pairs, thresholds=th, stats=stats) == want_pairs and stats["gpu_decodes"] == 6, stats
    assert [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)] == want_tiles
