"""The oversize refine route on the GPU (KE_GPU_REFINE_OVERSIZE=1): ke_jpeg_decode_scaled over the grid of
tests/_jpeg_scaled_cases.py in one shuffled batch of mixed denominators with guard bytes behind every image, ke_reduce_rgb and
ke_thumbnail_rgb_box against Pillow on the reduce set, and refine_pairs at max_side = 64 on the chain set, with the variable set
and unset.  No tolerances: bytes and SSIM values are equal or the test fails.  Small shapes only (no file is over 1100 px)."""
from __future__ import annotations

import io
import os

import numpy as np
import pytest
from PIL import Image

import _jpeg_scaled_cases as S

pytestmark = pytest.mark.gpu
GUARD = 32


def _native():
    from kobato_eyes_amd import _native

    return _native


@pytest.fixture(scope="module")
def ctx():
    return _native().get_context(0)


def _decode_scaled_with_guards(ctx, blobs, denoms):
    """ke_jpeg_decode_scaled into a buffer of its own whose images lie at every alignment with GUARD bytes of 0xA5 behind each:
    the per-file status, the images and the guards as the call left them."""
    K = _native()
    denoms = np.ascontiguousarray(denoms, np.int32)
    with ctx._lock:
        files = ctx._packed(blobs)
        w, h, c, st = ctx._probe(files, "jpeg")
        assert (st == 0).all()
        w, h = (w + denoms - 1) // denoms, (h + denoms - 1) // denoms
        nbytes = w.astype(np.int64) * h * c
        off = np.zeros(len(blobs), np.uint64)
        at = 0
        for k, nb in enumerate(nbytes.tolist()):
            off[k] = at
            at += nb + GUARD + k % 7
        host = np.full(at + 64, 0xA5, np.uint8)
        dev = ctx.malloc(host.nbytes)
        try:
            ctx.memcpy(dev, host, host.nbytes)
            ctx._check(ctx._lib.ke_jpeg_decode_scaled(ctx._h, K._addr(files.flat), K._addr(files.offsets), K._addr(files.sizes), len(blobs),
                                                      K._addr(denoms), dev, K._addr(off), K._addr(st)), "ke_jpeg_decode_scaled")
            ctx.memcpy(host, dev, host.nbytes)
        finally:
            ctx.free(dev)
    images, guards = [], []
    for k, nb in enumerate(nbytes.tolist()):
        o = int(off[k])
        images.append(host[o:o + nb].reshape((int(h[k]), int(w[k])) if c[k] == 1 else (int(h[k]), int(w[k]), int(c[k]))))
        guards.append(host[o + nb:o + nb + GUARD])
    return st, images, guards


def test_the_grid_in_one_shuffled_batch_of_mixed_denominators(ctx):
    files, reference = S.grid(), S.grid_reference()
    entries = [(i, ran, ref) for (i, _), (ref, ran) in reference.items()]
    order = np.random.default_rng(12).permutation(len(entries)).tolist()
    entries = [entries[k] for k in order]
    st, images, guards = _decode_scaled_with_guards(ctx, [files[i][1] for i, _, _ in entries], [d for _, d, _ in entries])
    assert {d for _, d, _ in entries} == {1, 2, 4, 8}
    wrong = [(files[i][0], d, int(s)) for (i, d, ref), s, px in zip(entries, st.tolist(), images) if s != 0 or px.shape != ref.shape or not np.array_equal(px, ref)]
    assert not wrong, (len(wrong), wrong[:20])
    assert all((g == 0xA5).all() for g in guards), "bytes behind an image were written"
    # denominator 1 is ke_jpeg_decode: the same bytes, file by file
    plain, status = ctx.jpeg_decode([data for _, data in files])
    assert (status == 0).all()
    seen = 0
    for (i, d, _), px in zip(entries, images):
        if d == 1:
            assert np.array_equal(px, plain[i]), files[i][0]
            seen += 1
    assert seen >= len(files)


def test_denominators_other_than_1_2_4_8_are_refused(ctx):
    K = _native()
    with ctx._lock, pytest.raises(Exception, match="scale 1/3"):
        files = ctx._packed([S.grid()[0][1]])
        dev = ctx.malloc(4096)
        try:
            st = np.zeros(1, np.int32)
            ctx._check(ctx._lib.ke_jpeg_decode_scaled(ctx._h, K._addr(files.flat), K._addr(files.offsets), K._addr(files.sizes), 1,
                                                      K._addr(np.array([3], np.int32)), dev, K._addr(np.zeros(1, np.uint64)), K._addr(st)),
                       "ke_jpeg_decode_scaled")
        finally:
            ctx.free(dev)


def test_draft_decode_picks_the_loaders_scale(ctx):
    blobs = [data for name, suffix, data in S.chain_files() if suffix == ".jpg"][::4]
    out, st, denoms = ctx.jpeg_decode_scaled(blobs, max_side=S.CHAIN_MAX_SIDE)
    assert (st == 0).all() and set(denoms.tolist()) == {1, 2, 4, 8}
    for data, px, d in zip(blobs, out, denoms.tolist()):
        ref, ran = S.pillow_at_scale(data, d)
        assert ran == d == S.draft_scale(*Image.open(io.BytesIO(data)).size, S.CHAIN_MAX_SIDE)
        assert np.array_equal(px, ref)


def test_reduce_and_boxed_thumbnail_equal_pillow(ctx):
    LANCZOS = Image.Resampling.LANCZOS
    cases = list(S.reduce_cases())
    top = max(a.size for *_, a in cases)
    src = ctx.malloc(top + 64)
    try:
        for w, h, fx, fy, a in cases:
            ctx.memcpy(src, np.ascontiguousarray(a), a.size)
            reduced = Image.fromarray(a).reduce((fx, fy))
            small, sw, sh = ctx.reduce_rgb(src, w, h, fx, fy)
            try:
                assert (sw, sh) == reduced.size
                got = np.empty((sh, sw, 3), np.uint8)
                ctx.memcpy(got, small, got.nbytes)
                assert np.array_equal(got, np.asarray(reduced)), ("reduce", w, h, fx, fy)
                # the resample thumbnail runs next: through the fractional box (0, 0, w / fx, h / fy) of the reduced image
                tw, th = max(1, sw * 2 // 3), max(1, sh * 2 // 3)
                box = (0.0, 0.0, w / fx, h / fy)
                ref = np.asarray(reduced.resize((tw, th), LANCZOS, box=box, reducing_gap=None))
                thumb = ctx.thumbnail_rgb_box(small, sw, sh, tw, th, box)
                try:
                    got = np.empty((th, tw, 3), np.uint8)
                    ctx.memcpy(got, thumb, got.nbytes)
                finally:
                    ctx.free(thumb)
                assert np.array_equal(got, ref), ("box", w, h, fx, fy, tw, th)
            finally:
                ctx.free(small)
    finally:
        ctx.free(src)


def test_thumbnail_rgb_reduced_is_image_thumbnail(ctx):
    m = S.CHAIN_MAX_SIDE
    factors = set()
    for k, (w, h) in enumerate(S.CHAIN_SIZES + tuple((h, w) for w, h in S.CHAIN_SIZES if w != h)):      # ... and as a turn leaves them
        a = S.smooth(w, h, 300 + k)
        ref = Image.fromarray(a)
        ref.thumbnail((m, m), Image.Resampling.LANCZOS)
        src = ctx.malloc(a.size + 64)
        try:
            ctx.memcpy(src, a, a.size)
            dev, tw, th, f = ctx.thumbnail_rgb_reduced(src, w, h, m)
            try:
                assert (tw, th) == ref.size
                got = np.empty((th, tw, 3), np.uint8)
                ctx.memcpy(got, dev, got.nbytes)
            finally:
                ctx.free(dev)
        finally:
            ctx.free(src)
        assert np.array_equal(got, np.asarray(ref)), (w, h, f)
        factors.add(f)
    assert factors >= S.CHAIN_FACTORS


@pytest.fixture(scope="module")
def chain_pairs(tmp_path_factory):
    """[(id a, id b, path a, path b)] over the chain set: every file with the next one, and every JPEG with the PNG of its size."""
    root = tmp_path_factory.mktemp("oversize_chain")
    paths = []
    for name, suffix, data in S.chain_files():
        p = root / (name + suffix)
        p.write_bytes(data)
        paths.append(str(p))
    pairs = [(k, k + 1, a, b) for k, (a, b) in enumerate(zip(paths, paths[1:]))]
    pairs += [(k, 5 * (k // 5) + 4, paths[k], paths[5 * (k // 5) + 4]) for k in range(len(paths)) if k % 5 != 4]
    return paths, pairs


def test_refine_pairs_takes_the_oversize_files_and_scores_them_as_the_loader_does(chain_pairs, monkeypatch):
    import kobato_eyes_amd as K
    from kobato_eyes_amd.image_io import safe_load_image

    paths, pairs = chain_pairs
    m = S.CHAIN_MAX_SIDE
    monkeypatch.delenv("KE_GPU_REFINE_OVERSIZE", raising=False)
    before: dict = {}
    loader = K.refine_pairs(pairs, max_side=m, stats=before)
    assert before.get("gpu_oversize", 0) == 0 and before["gpu_decodes"] == 0       # every file here is past the window at 64
    monkeypatch.setenv("KE_GPU_REFINE_OVERSIZE", "1")
    after: dict = {}
    got = K.refine_pairs(pairs, max_side=m, stats=after)
    assert after["gpu_oversize"] == len(paths) == after["gpu_decodes"], after
    assert len(got) == len(loader) == len(pairs)
    for (a, b, pa, pb), x, y in zip(pairs, got, loader):
        assert x is not None and y is not None, (pa, pb)
        assert x.ssim == y.ssim, (pa, pb, x.ssim, y.ssim)
        assert x == y
    # the yardstick itself: the loader's pixels of the same pairs through the SSIM entry for host images
    ctx = _native().get_context(0)
    images = [np.asarray(safe_load_image(p, max_side=m)) for p in paths]
    index = {p: k for k, p in enumerate(paths)}
    scores, status = ctx.ssim_pairs(images, [index[pa] for _, _, pa, _ in pairs], [index[pb] for _, _, _, pb in pairs])
    # (a 64 x 8 thumbnail against a 6 x 64 one has no 7 x 7 window: no value, on either route)
    assert [float(s) if st == 0 else None for s, st in zip(scores, status)] == [x.ssim for x in got]
    narrow =[any(os.path.basename(p).startswith("64x700") for p in (pa, pb)) for _, _, pa, pb in pairs]
    assert [x.ssim is None for x in got] == narrow and sum(narrow) < len(pairs) // 4
