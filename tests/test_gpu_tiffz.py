"""ke_tiffz_decode on the GPU: deflate-compressed TIFF files against Pillow / libtiff and the CPU build's rule, bit for bit --
every taken and every CORRUPT case in one shuffled batch; a file of 130 strips at every alignment; long strips; one bad strip
among good files; sub-batches; the hashes; the batch hasher and the refine seams with KE_GPU_TIFF_DEFLATE set and unset.
Every call is one bounded batch of small files."""
from __future__ import annotations

import io
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
from PIL import Image

import _tiff_cases as T
import _tiffc_cases as A
import _tiffz_cases as Z
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
        ref = Z.pillow_pixels(data)
        assert st == Z.OK, (name, st)
        assert px.shape == ref.shape, (name, px.shape, ref.shape)
        assert np.array_equal(px, ref), name


def test_every_case_in_one_shuffled_batch(ctx):
    """Every valid file, every refusal and every CORRUPT case -- the two rows where the decoder is stricter than libtiff among
    them -- in one call: the statuses are the CPU build's (tests/test_tiffz_cpu.py holds those to Pillow), the pixels Pillow's."""
    cases = [(n, d, Z.OK) for _, n, d in Z.valid_cases()] + Z.refused_cases() + [(n, d, Z.CORRUPT) for n, d, _ in Z.corrupt_cases()]
    order = np.random.default_rng(7).permutation(len(cases))
    out, status = ctx.tiffz_decode([cases[k][1] for k in order])
    shapes = set()
    for k, px, st in zip(order.tolist(), out, status):
        name, data, expected = cases[k]
        assert st == expected, (name, st)
        if expected != Z.OK:
            assert px is None, name
            continue
        ref = Z.pillow_pixels(data)
        assert px.shape == ref.shape, (name, px.shape, ref.shape)
        assert np.array_equal(px, ref), name
        shapes.add(ref.shape[2] if ref.ndim == 3 else 1)
    assert sum(e == Z.OK for _, _, e in cases) > 500 and sum(e == Z.CORRUPT for _, _, e in cases) > 30 and shapes == {1, 3, 4}


def test_probe_reports_what_pillow_opens(ctx):
    cases = Z.pillow_cases()[::3] + Z.handmade_cases()[::5]
    w, h, c, st = ctx.tiffz_probe([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        ref = Z.pillow_pixels(data)
        assert st[k] == 0 and (h[k], w[k]) == ref.shape[:2] and c[k] == (ref.shape[2] if ref.ndim == 3 else 1), name


def test_three_groups_of_strips_at_every_alignment(ctx):
    """130 x 130 RGB in strips of 1 row: 130 strips, three groups of 64 in the list.  Sixteen such files, each with a byte behind
    its directory (the writer puts strips at even offsets; the byte makes every other file start at an odd one), so that the
    strips of the call start at every offset modulo 16 -- the uploaded bytes start where the first file starts."""
    rng = np.random.default_rng(11)
    a = np.ascontiguousarray(Z.content(rng, 130, 130, "smooth")[..., :3])
    files, starts = [], set()
    at = 0
    for pad in range(16):
        text = bytes(rng.integers(65, 91, 5 + pad, dtype=np.uint8)) + b"\0"
        data = Z.compressed(a, Z.DEFLATE, rows=1, predictor=2, encode=lambda d: zlib.compress(d, 1 + pad % 9), more=[(305, 2, len(text), text)]) + b"\0"
        starts |= {(at + off) % 16 for off, _ in A._regions(data)[1]}
        at += len(data)
        files.append((f"pad_{pad}", data))
    assert starts == set(range(16))
    out, status = ctx.tiffz_decode([d for _, d in files])
    _check(files, out, status)
    assert ctx.tiffz_probe([files[0][1]])[3][0] == 0 and len(A._regions(files[0][1])[1]) == 130


def test_long_strips(ctx):
    """The 331 x 100 gray file with matches at distance 32 768, and 1 100 x 1 000 gray, all 255, in one strip: 1.1 MB of runs at
    distance 1 in about 4 300 symbols, and an Adler sum that overflows 32 bits unless it is reduced on the way."""
    far = dict(Z.named_stream_cases())["match_at_distance_32768"]
    white = Z.compressed(np.full((1000, 1100), 255, np.uint8), Z.DEFLATE, encode=lambda d: zlib.compress(d, 9))
    assert len(A._regions(white)[1]) == 1
    files = [("far", far), ("white", white)]
    out, status = ctx.tiffz_decode([d for _, d in files])
    _check(files, out, status)


def test_one_bad_strip_between_good_files(ctx):
    """A 13-strip file (512 x 512 RGB as libtiff cuts it: 42 rows a strip) whose strip 7 alone has a wrong trailer, between two
    good files: status 2, not one of its pixels written, the neighbours right."""
    rng = np.random.default_rng(12)
    a = np.ascontiguousarray(Z.content(rng, 512, 512, "smooth")[..., :3])
    count = [0]

    def encode(d, bad):
        z = zlib.compress(d, 1)
        count[0] += 1
        return z[:-1] + bytes([z[-1] ^ 1]) if bad and count[0] == 8 else z

    good = Z.compressed(a, Z.DEFLATE, rows=42, encode=lambda d: encode(d, False))
    count[0] = 0
    bad = Z.compressed(a, Z.DEFLATE, rows=42, encode=lambda d: encode(d, True))
    assert len(A._regions(bad)[1]) == 13 and Z.pillow_pixels(bad) is None
    other = Z.pillow_file(Z.content(rng, 200, 150, "drawing"), "RGB", "tiff_adobe_deflate", True)
    blobs = [good, bad, other]
    with ctx._lock:
        dev, off, w, h, c, st, _ = ctx._decode_packed(ctx._packed(blobs), "tiffz")
        assert st.tolist() == [0, 2, 0]
        # the decode buffer as the call left it: the good files' pixels, and between them whatever was there before
        got = [np.empty(512 * 512 * 3, np.uint8), np.empty(200 * 150 * 3, np.uint8)]
        ctx.memcpy(got[0], dev + int(off[0]), got[0].nbytes)
        ctx.memcpy(got[1], dev + int(off[2]), got[1].nbytes)
        # fill the bad file's place with a pattern, decode again: the pattern is still there
        n = int(w[1]) * int(h[1]) * int(c[1])
        assert (int(w[1]), int(h[1]), int(c[1])) == (512, 512, 3)
        pattern = np.full(n, 0xA5, np.uint8)
        ctx.memcpy(dev + int(off[1]), pattern, n)
        dev2, off2, _, _, _, st2, _ = ctx._decode_packed(ctx._packed(blobs), "tiffz")
        assert st2.tolist() == [0, 2, 0] and dev2 == dev and off2.tolist() == off.tolist()
        back = np.empty(n, np.uint8)
        ctx.memcpy(back, dev + int(off[1]), n)
    assert np.array_equal(back, pattern)
    assert np.array_equal(got[0].reshape(512, 512, 3), a) and np.array_equal(got[1].reshape(150, 200, 3), Z.pillow_pixels(other))


def test_sub_batches(ctx, monkeypatch):
    """40 files of 64 x 64 whole and cut into sub-batches: the same statuses and pixels, and the count of sub-batches the call
    reports.  Unset: one.  64 KiB: several, with several files in some (a gray file's plane is 4 KiB, an RGBA file's 16 KiB
    plus records, streams and 10 KiB of header work for one wave).  1 byte: no two files fit, one sub-batch per file."""
    rng = np.random.default_rng(13)
    cases = []
    for k in range(40):
        mode = ("L", "RGB", "RGBA", "P")[k % 4]
        cases.append((f"f{k}", Z.pillow_file(Z.content(rng, 64, 64, ("noise", "smooth", "drawing")[k % 3]), mode, "tiff_adobe_deflate", k % 2 == 1)))
    cases[17] = ("cut", Z.compressed(np.ascontiguousarray(Z.content(rng, 64, 64, "smooth")[..., :3]), Z.DEFLATE, rows=16, encode=lambda d: zlib.compress(d)[:-2]))
    monkeypatch.delenv("KE_TIFFZ_SCRATCH_BYTES", raising=False)
    whole, st_whole = ctx.tiffz_decode([d for _, d in cases])
    assert ctx.last_decode_sub_batches() == 1
    monkeypatch.setenv("KE_TIFFZ_SCRATCH_BYTES", "1")
    singles, st_singles = ctx.tiffz_decode([d for _, d in cases])
    assert ctx.last_decode_sub_batches() == 40 and st_singles.tolist() == st_whole.tolist()
    assert all(np.array_equal(whole[k], singles[k]) for k in range(40) if k != 17)
    monkeypatch.setenv("KE_TIFFZ_SCRATCH_BYTES", str(1 << 16))
    parts, st_parts = ctx.tiffz_decode([d for _, d in cases])
    assert 3 <= ctx.last_decode_sub_batches() < 40
    assert st_whole.tolist() == st_parts.tolist() == [2 if k == 17 else 0 for k in range(40)]
    keep = [k for k in range(40) if k != 17]
    _check([cases[k] for k in keep], [parts[k] for k in keep], [st_parts[k] for k in keep])
    assert all(np.array_equal(whole[k], parts[k]) for k in keep)


def test_hash_equals_the_oracle_of_pillow_pixels(ctx):
    cases = [(n, d) for n, d in Z.pillow_cases() if min(Z.pillow_pixels(d).shape[:2]) >= 8]
    ph, dh, st = ctx.hash([d for _, d in cases], kind="tiffz")
    for k, (name, data) in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(Z.pillow_pixels(data)), name
    assert len(cases) >= 60


def test_damage_is_refused_or_equal_to_pillow(ctx):
    """The damaged set of tests/test_tiffz_cpu.py through the kernels in one batch: taken => strict Pillow takes the file with
    equal pixels.  The floor is that test's (32; its docstring derives it)."""
    files = Z.damaged_set()
    out, status = ctx.tiffz_decode(files)
    taken = 0
    for k, (data, px, st) in enumerate(zip(files, out, status)):
        assert st in (Z.OK, Z.UNSUPPORTED, Z.CORRUPT)
        if st == Z.OK:
            ref = Z.pillow_pixels(data)
            taken += 1
            assert ref is not None and px.shape == ref.shape and np.array_equal(ref, px), k
    print(f"damage census through the kernels: {len(files)} cases, the decoder takes {taken}")
    assert len(files) == 2400 and taken >= 32


def _write(tmp_path, cases, first=0, suffix=".tif"):
    items = []
    for k, (_, data) in enumerate(cases):
        p = tmp_path / f"{first + k:03d}{suffix}"
        p.write_bytes(data)
        items.append((900 + first + k, str(p)))
    return items


def test_batch_hasher_rows_with_the_deflate_route_on_and_off(tmp_path, monkeypatch):
    """JPEG, uncompressed, LZW and deflate TIFF files in one run: the same rows with KE_GPU_TIFF_DEFLATE=1 as without it, and the
    deflate files reach the Pillow share only when it is unset (LZW files always: KE_GPU_TIFF_COMPRESSED stays unset)."""
    from kobato_eyes_amd import fastsig as K

    big_enough = lambda d: min(Z.pillow_pixels(d).shape[:2]) >= 8
    rng = np.random.default_rng(14)
    jpegs = []
    for k in range(8):
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(Z.content(rng, 96, 80, "smooth")[..., :3])).save(b, "JPEG", quality=85)
        jpegs.append((f"j{k}", b.getvalue()))
    plain = [(n, d) for n, d, _ in T.supported() if big_enough(d)][:10]
    lzw = [(n, d) for n, d in A.pillow_cases() if "lzw" in n and big_enough(d)][:8]
    packed = [(n, d) for n, d in Z.pillow_cases() + Z.handmade_cases()[30::7] if big_enough(d)][:34]
    others = [(n, d) for n, d, _ in Z.refused_cases() if n in ("orientation_6_deflate", "predictor_3_deflate")] + \
             [(n, d) for n, d, _, opens in Z.odd_strip_cases() if opens and n.startswith(Z.STRICTER_THAN_LIBTIFF)][:3]
    items = _write(tmp_path, jpegs, suffix=".jpg") + _write(tmp_path, plain + lzw + packed + others, first=len(jpegs))
    group = lambda lo, n: {p for _, p in items[lo:lo + n]}
    at = len(jpegs)
    plain_paths, lzw_paths = group(at, len(plain)), group(at + len(plain), len(lzw))
    packed_paths, other_paths = group(at + len(plain) + len(lzw), len(packed)), group(at + len(plain) + len(lzw) + len(packed), len(others))
    seen = []
    original = K._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        seen.extend(self.paths[k] for k in todo)
        return original(self, todo, out)

    monkeypatch.setattr(K._Pipeline, "_decode_with_pillow", spy)
    for v in ("KE_GPU_TIFF_DEFLATE", "KE_GPU_TIFF_COMPRESSED"):
        monkeypatch.delenv(v, raising=False)
    rows = K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert packed_paths | other_paths | lzw_paths <= set(seen) and not plain_paths & set(seen)
    assert len(rows) >= len(jpegs) + len(plain) + len(lzw) + len(packed) and len(items) >= 60
    monkeypatch.setenv("KE_GPU_TIFF_DEFLATE", "1")
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert not (packed_paths | plain_paths) & set(seen), "a file the GPU decoders take went to the Pillow share"
    assert other_paths | lzw_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_TIFF", "0")                                   # the whole TIFF route off: the variable alone does nothing
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert packed_paths | plain_paths <= set(seen)


def test_refine_seams_with_the_deflate_route_on_and_off(tmp_path, monkeypatch):
    import kobato_eyes_amd as KA
    from kobato_eyes_amd import refine_parallel as RP

    rng = np.random.default_rng(3)
    base = O.synth_rgb(4242, 96, 80)
    files = []
    for k in range(8):
        px = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) if k % 2 else base
        if k in (2, 5):                                                  # an orientation to apply: the loader's
            data = Z.compressed(px, Z.DEFLATE, rows=16, encode=zlib.compress, more=[(274, 3, 1, [6])])
        else:
            data = Z.pillow_file(np.dstack([px, px[..., :1]]), "RGB", "tiff_adobe_deflate" if k % 4 else "tiff_deflate", k % 3 == 0)
        p = tmp_path / f"t{k}.tif"
        p.write_bytes(data)
        files.append(p)
    for v in ("KE_GPU_TIFF_DEFLATE", "KE_GPU_TIFF_COMPRESSED"):
        monkeypatch.delenv(v, raising=False)
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
    monkeypatch.setenv("KE_GPU_TIFF_DEFLATE", "1")
    on_gpu = RP._thumbnails_decoded_on_gpu(files, 32, 0)
    assert set(on_gpu) == {p for k, p in enumerate(files) if k not in (2, 5)}
    for p, t in on_gpu.items():
        assert np.array_equal(t, RP._thumbnails([RP._decode(p)], 32, 0)[0]), p
    stats = {}
    assert KA.refine_pairs(pairs, thresholds=th, stats=stats) == want_pairs and stats["gpu_decodes"] == 6, stats
    assert [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)] == want_tiles
