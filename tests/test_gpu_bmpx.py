"""ke_bmpx_decode on the GPU: RLE, 1 / 4-bit and 16-bit BMP files against Pillow and the CPU build's statuses, bit for bit -- every
valid, invalid and random case in one shuffled batch with guard bytes behind every plane; the same batch in sub-batches; one
larger file of each kind and a wide row; the hashes; the batch hasher and the refine seams with KE_GPU_BMP_EXTENDED set and
unset.  Every call is one bounded batch of small files."""
from __future__ import annotations

import ctypes as C
import io
import os
import shutil
import subprocess
from dataclasses import dataclass

import numpy as np
import pytest
from PIL import Image

import _bmp_cases as B
import _bmpx_cases as X
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 48


def _native():
    from kobato_eyes_amd import _native

    return _native


@pytest.fixture(scope="module")
def ctx():
    return _native().get_context(0)


@pytest.fixture(scope="module")
def cpu_status(tmp_path_factory):
    """The CPU build's word on a file (tests/test_bmpx_cpu.py holds it to Pillow)."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("bmpx_cpu") / "bmpx_cpu.so")
    subprocess.check_call([cxx, "-std=c++17", "-shared", "-fPIC", "-O2", "-I", os.path.join(ROOT, "kobato-eyes_amd", "csrc"),
                           os.path.join(ROOT, "tests", "_bmpx_cpu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.bmpx_cpu_probe.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]
    lib.bmpx_cpu_decode.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p]

    def status(data: bytes) -> int:
        info = np.zeros(8, np.int32)
        lib.bmpx_cpu_probe(data, len(data), info.ctypes.data)
        if info[0] != 0:
            return int(info[0])
        out = np.zeros(int(info[1]) * int(info[2]) * int(info[3]), np.uint8)
        return int(lib.bmpx_cpu_decode(data, len(data), out.ctypes.data))

    return status


@pytest.fixture(scope="module")
def everything(cpu_status):
    """[(name, file, the CPU build's status, Pillow's pixels or None)] of every set, computed once."""
    return [(n, d, cpu_status(d), X.pillow_pixels(d)) for n, d in X.every_file()]


def _decode_with_guards(ctx, blobs):
    """ke_bmpx_decode into a buffer of its own whose planes lie at every alignment with GUARD bytes of 0xA5 behind each: the
    per-file status, the planes and the guards as the call left them."""
    K = _native()
    with ctx._lock:
        files = ctx._packed(blobs)
        w, h, c, st = ctx._probe(files, "bmpx")
        nbytes = np.where(st == 0, w.astype(np.int64) * h * c, 0)
        off = np.zeros(len(blobs), np.uint64)
        at = 0
        for k, nb in enumerate(nbytes.tolist()):
            off[k] = at
            at += nb + GUARD + k % 7                                   # planes start at every alignment
        host = np.full(at + 64, 0xA5, np.uint8)
        dev = ctx.malloc(host.nbytes)
        try:
            ctx.memcpy(dev, host, host.nbytes)
            ctx._check(ctx._lib.ke_bmpx_decode(ctx._h, K._addr(files.flat), K._addr(files.offsets), K._addr(files.sizes), len(blobs), dev,
                                               K._addr(off), K._addr(st)), "ke_bmpx_decode")
            sub_batches = ctx.last_decode_sub_batches()
            ctx.memcpy(host, dev, host.nbytes)
        finally:
            ctx.free(dev)
    planes, guards = [], []
    for k, nb in enumerate(nbytes.tolist()):
        o = int(off[k])
        shape = (int(h[k]), int(w[k])) if c[k] == 1 else (int(h[k]), int(w[k]), int(c[k]))
        planes.append(host[o:o + nb].reshape(shape) if nb else None)
        guards.append(host[o + nb:o + nb + GUARD])
    return st, planes, guards, sub_batches


def _hold(everything, order, st, planes, guards):
    for k, s, px, guard in zip(order, st.tolist(), planes, guards):
        name, data, expected, ref = everything[k]
        assert s == expected, (name, s, expected)
        assert (guard == 0xA5).all(), f"{name}: bytes behind the plane were written"
        if s == X.OK:
            assert px.shape == ref.shape, (name, px.shape, ref.shape)
            assert np.array_equal(px, ref), name


def test_every_case_in_one_shuffled_batch(ctx, everything, monkeypatch):
    """Every valid, invalid and random case in one call: the statuses are the CPU build's, the pixels Pillow's, and the guard
    bytes behind every image's plane -- also behind the planes of streams that fall short -- are untouched."""
    monkeypatch.delenv("KE_BMPX_SCRATCH_BYTES", raising=False)
    order = np.random.default_rng(7).permutation(len(everything)).tolist()
    st, planes, guards, sub_batches = _decode_with_guards(ctx, [everything[k][1] for k in order])
    _hold(everything, order, st, planes, guards)
    expected = np.array([everything[k][2] for k in order])
    assert sub_batches == 1 and (expected == 0).sum() > 1300 and (expected == 2).sum() > 200 and (expected == 1).sum() > 30


def test_the_same_batch_in_sub_batches(ctx, everything, monkeypatch):
    """KE_BMPX_SCRATCH_BYTES small enough for three sub-batches and more -- the record scratch of the whole batch is about 1.5 MB
    (16 bytes per two bytes of stream) --: the same statuses and pixels, and the count the call reports."""
    order = np.random.default_rng(8).permutation(len(everything)).tolist()
    blobs = [everything[k][1] for k in order]
    monkeypatch.setenv("KE_BMPX_SCRATCH_BYTES", str(200_000))
    st, planes, guards, sub_batches = _decode_with_guards(ctx, blobs)
    assert 3 <= sub_batches < 100, sub_batches
    _hold(everything, order, st, planes, guards)
    monkeypatch.setenv("KE_BMPX_SCRATCH_BYTES", "1")               # no two RLE files fit: a sub-batch ends behind every one
    few = blobs[:120]
    st1, planes1, guards1, singles = _decode_with_guards(ctx, few)
    assert st1.tolist() == st[:120].tolist() and singles >= sum(n.startswith(("rle", "random")) for n, *_ in (everything[k] for k in order[:120])) > 60
    assert all(np.array_equal(a, b) for a, b in zip(planes1, planes[:120]) if a is not None)


def test_probe_reports_what_pillow_opens(ctx):
    cases = [(n, d) for n, d, _ in X.valid_cases()][::7]
    w, h, c, st = ctx.bmpx_probe([d for _, d in cases])
    for k, (name, data) in enumerate(cases):
        ref = X.pillow_pixels(data)
        assert st[k] == 0 and (h[k], w[k]) == ref.shape[:2] and c[k] == (ref.shape[2] if ref.ndim == 3 else 1), name


def _larger_files():
    rng = np.random.default_rng(21)
    out = []
    for w, h in ((512, 512), (2049, 3)):
        drawing = Image.fromarray(np.ascontiguousarray(X.content(rng, w, h, "drawing")[..., :3]))
        photo = Image.fromarray(np.ascontiguousarray(X.content(rng, w, h, "smooth")[..., :3]))
        for kind, n in (("rle8", 256), ("rle4", 16), ("p4", 16), ("p1", 2)):
            for what, im in (("drawing", drawing), ("photo", photo)):
                q = im.quantize(n)
                pal = np.asarray(q.getpalette()[:3 * n], np.uint8).reshape(-1, 3)
                pal = np.concatenate([pal[:, ::-1], np.full((len(pal), 1), 0, np.uint8)], 1)
                pal[0, :3] = (12, 40, 90)
                out.append((f"{kind}_{what}_{w}x{h}", X.picture(kind, np.asarray(q), pal=pal.tobytes(), topdown=what == "photo" and kind == "rle8")))
        noise = rng.integers(0, 256, (h, w)).astype(np.uint8)
        out.append((f"rle8_noise_{w}x{h}", X.picture("rle8", noise, pal=X.palette(rng, 256))))
        px = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        for kind in ("rgb555", "rgb555m", "rgb565"):
            out.append((f"{kind}_{w}x{h}", X.picture(kind, px, hs=124 if kind == "rgb565" else 40)))
    return out


def test_one_larger_file_of_each_kind(ctx):
    """512 x 512 of every kind -- drawing-like, photograph-like and noise: streams of 2 KB to 270 KB, chunks of records beyond one
    workgroup -- and 2049 x 3 for the rows that are wider than a workgroup's stride."""
    files = _larger_files()
    out, status = ctx.bmpx_decode([d for _, d in files])
    for (name, data), px, st in zip(files, out, status):
        ref = X.pillow_pixels(data)
        assert st == X.OK, (name, st)
        assert px.shape == ref.shape and np.array_equal(px, ref), name
    assert len(files) == 2 * (8 + 1 + 3)


def test_hash_equals_the_hash_of_pillows_pixels(ctx):
    cases = [(n, d) for n, d, _ in X.valid_cases() if min(X.pillow_pixels(d).shape[:2]) >= 8] + [(n, d) for n, d in _larger_files() if "512x512" in n]
    ph, dh, st = ctx.bmpx_hash([d for _, d in cases])
    assert (st == 0).all()
    for channels in (1, 3):
        pick = [k for k, (_, d) in enumerate(cases) if (X.pillow_pixels(d).ndim == 3) == (channels == 3)]
        ref_p, ref_d, ref_st = ctx.hash_images([np.ascontiguousarray(X.pillow_pixels(cases[k][1])) for k in pick])
        assert (ref_st == 0).all() and len(pick) >= 13
        assert np.array_equal(ph[pick], ref_p) and np.array_equal(dh[pick], ref_d), channels
    name, data = cases[0]
    assert (int(ph[0]), int(dh[0])) == O.hash_image(X.pillow_pixels(data)), name


def _write(tmp_path, cases, first=0, suffix=".bmp"):
    items = []
    for k, (_, data) in enumerate(cases):
        p = tmp_path / f"{first + k:03d}{suffix}"
        p.write_bytes(data)
        items.append((900 + first + k, str(p)))
    return items


def test_batch_hasher_rows_with_the_extended_route_on_and_off(tmp_path, monkeypatch):
    """JPEG files and BMP files of every kind in one run: the same rows with KE_GPU_BMP_EXTENDED=1 as without it, and the files
    ke_bmpx_decode takes reach the Pillow share only when it is unset."""
    from kobato_eyes_amd import fastsig as K

    big_enough = lambda d: min(X.pillow_pixels(d).shape[:2]) >= 8
    rng = np.random.default_rng(14)
    jpegs = []
    for k in range(6):
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(X.content(rng, 96, 80, "smooth")[..., :3])).save(b, "JPEG", quality=85)
        jpegs.append((f"j{k}", b.getvalue()))
    plain = [(n, d) for n, d, _ in B.supported() if big_enough(d)][:10]
    taken = [(n, d) for n, d, _ in X.valid_cases() if "picture" in n or "every_value" in n or n.endswith("_topdown")]
    taken = [(n, d) for n, d in taken if big_enough(d)] + [(n, d) for n, d in _larger_files() if "512x512" in n]
    by_name = {n: d for n, d, _ in X.invalid_cases()}
    others = [(n, by_name[n]) for n in ("rle8_with_4_bits", "rle4_with_8_bits", "unknown_16_bit_masks_0_hs40",       # refused: status 1
                                        "rle8_early_end_of_bitmap", "rle4_pixels_short_by_one", "rle8_cut_inside_a_delta")]    # fall short: status 2
    items = _write(tmp_path, jpegs, suffix=".jpg") + _write(tmp_path, plain + taken + others, first=len(jpegs))
    group = lambda lo, n: {p for _, p in items[lo:lo + n]}
    at = len(jpegs)
    plain_paths, taken_paths, other_paths = group(at, len(plain)), group(at + len(plain), len(taken)), group(at + len(plain) + len(taken), len(others))
    seen = []
    original = K._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        seen.extend(self.paths[k] for k in todo)
        return original(self, todo, out)

    monkeypatch.setattr(K._Pipeline, "_decode_with_pillow", spy)
    monkeypatch.delenv("KE_GPU_BMP_EXTENDED", raising=False)
    monkeypatch.delenv("KE_GPU_BMP", raising=False)
    rows = K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert taken_paths | other_paths <= set(seen) and not plain_paths & set(seen)
    assert len(rows) >= len(jpegs) + len(plain) + len(taken) and len(items) >= 60
    monkeypatch.setenv("KE_GPU_BMP_EXTENDED", "1")
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert not (taken_paths | plain_paths) & set(seen), "a file the GPU decoders take went to the Pillow share"
    assert other_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_BMP", "0")                                    # the whole BMP route off: the variable alone does nothing
    seen.clear()
    assert rows == K.compute_signatures_mp(items, max_workers=4, chunksize=16)
    assert taken_paths | plain_paths <= set(seen)


def test_refine_seams_with_the_extended_route_on_and_off(tmp_path, monkeypatch):
    import kobato_eyes_amd as KA
    from kobato_eyes_amd import refine_parallel as RP

    rng = np.random.default_rng(3)
    base = O.synth_rgb(4242, 96, 80)
    files = []
    for k in range(8):
        px = np.clip(base.astype(np.int16) + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) if k % 2 else base
        if k in (2, 5):                                                  # a palette file: luma only, the hashing seams' and the thumbnails'
            q = Image.fromarray(px).quantize(256)
            pal = np.asarray(q.getpalette()[:768], np.uint8).reshape(-1, 3)
            data = X.picture("rle8", np.asarray(q), pal=np.concatenate([pal[:, ::-1], np.zeros((256, 1), np.uint8)], 1).tobytes())
        else:
            p16 = px.astype(np.uint16)
            if k % 4 == 0:
                data = X.picture("rgb555", (p16[..., 0] >> 3 << 10) | (p16[..., 1] >> 3 << 5) | (p16[..., 2] >> 3), topdown=k == 4)
            else:
                data = X.picture("rgb565", (p16[..., 0] >> 3 << 11) | (p16[..., 1] >> 2 << 5) | (p16[..., 2] >> 3))
        p = tmp_path / f"t{k}.bmp"
        p.write_bytes(data)
        files.append(p)
    monkeypatch.delenv("KE_GPU_BMP_EXTENDED", raising=False)
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
    monkeypatch.setenv("KE_GPU_BMP_EXTENDED", "1")
    on_gpu = RP._thumbnails_decoded_on_gpu(files, 32, 0)
    assert set(on_gpu) == set(files)
    for p, t in on_gpu.items():
        assert np.array_equal(t, RP._thumbnails([RP._decode(p)], 32, 0)[0]), p
    stats = {}
    assert KA.refine_pairs(pairs, thresholds=th, stats=stats) == want_pairs and stats["gpu_decodes"] == 6, stats
    assert [[c.keeper_id, [e.file.file_id for e in c.files]] for c in KA.refine_by_tilehash_parallel(clusters, grid=4, tile=8, io_workers=2)] == want_tiles
