"""The host side the GPU decoders share (csrc/ke_decode_batch.h): accept, sort, pack into sub-batches, scatter the statuses.
One small mixed batch per kind, decoded in one call: decodable files of mixed shapes between files the parser refuses, cut
ones and an empty one, in shuffled order -- every index gets its own status and its own pixels.  Where a variable bounds the
sub-batches it is set so low that the batch is cut into three or more (held on the CPU against the decoders' cost formulas)."""
from __future__ import annotations

import numpy as np
import pytest

import _bmp_cases as B
import _gif_cases as GF
import _jpeg_cases as J
import _png_cases as P
import _tiff_cases as TF
import _tiffc_cases as TC
import _webp_cases as W
import _webpa_cases as A
import _webpl_cases as L

KINDS = ("jpeg", "png", "bmp", "gif", "tiff", "tiffc", "webp", "webpl", "webpa")
# the variable that bounds a sub-batch's scratch, and a value that cuts these few small images into three sub-batches or more
# with several images in some of them (sub_batches() below): a macroblock is 1 172 B of lossy-WebP scratch, a VP8L stream's memory
# 77 KB and more, an LZW strip's dictionaries 2 MB (such an image is a sub-batch of its own; the PackBits files pack together).
# A JPEG costs 128 B per block of coefficients plus its planes padded to 16: 192 B for 1 x 1 gray, 576 B for an 8 x 8 4:4:4 MCU,
# 1 536 B for 16 x 16 4:4:0 -- 2 000 B hold three of the second and none beside the third; the order within equal geometry is by
# the parsed scan length, so the count is held at run time.  A PNG costs its stream padded to 16, its filtered rows + 32 padded
# to 16 and 8 B per 3 of them + 16: 80 B (1 x 1 gray) to 264 B (7 x 5 gray) for the files below 64 x 64
BUDGET = {"jpeg": ("KE_JPEG_SCRATCH_BYTES", 2000), "png": ("KE_PNG_SCRATCH_BYTES", 400), "webp": ("KE_WEBP_SCRATCH_BYTES", 6000), "webpl": ("KE_WEBP_SCRATCH_BYTES", 250000),
          "webpa": ("KE_WEBP_SCRATCH_BYTES", 130000), "tiffc": ("KE_TIFFC_SCRATCH_BYTES", 8192)}
# the generators' cases that end early (status 2), by name.  jpeg's, png's and gif's, tiffc's lzw_short_strip, webpl's
# stream_ends_early and webpa's vp8l_plane_cut_in_half pass the header probe: the decode call itself finds the end, so a
# status that is not the parser's goes through the scatter
CUT = {"jpeg": ("truncated", "progressive_truncated"), "png": ("truncated",), "bmp": ("truncated_by_one", "truncated_half"),
       "gif": ("truncated_half", "truncated_in_the_last_block"), "tiff": ("strip_ends_behind_the_file",),
       "tiffc": ("file_cut_in_the_last_strip", "lzw_short_strip"), "webp": ("truncated_half", "truncated_header"),
       "webpl": ("truncated_half", "stream_ends_early"), "webpa": ("truncated_half", "vp8l_plane_cut_in_half")}
# an empty file: "not decodable" (2) from the parsers that read a signature first, "not mine" (1) from the WebP container walk
EMPTY = {k: 1 if k.startswith("webp") else 2 for k in KINDS}


def _material(kind: str):
    """([(name, file, Pillow's pixels as the format's own test converts them)], [(name, file, status)]) from the kind's generators."""
    if kind in ("jpeg", "png", "bmp", "gif", "tiff"):
        cases = {"jpeg": J, "png": P, "bmp": B, "gif": GF, "tiff": TF}[kind]
        return list(cases.supported()), [r for r in cases.refused() if r[2] is not None]
    if kind == "tiffc":
        return [(n, d, TC.pillow_pixels(d)) for n, d in TC.pillow_cases()], TC.refused_cases()
    if kind == "webp":
        return [(n, d, W.pillow_rgb(d)) for n, d in W.pillow_cases(n=40)], W.refused_cases()
    if kind == "webpl":
        return [(n, d, L.pillow_pixels(d)) for n, d in L.pillow_cases(n=40)], L.refused_cases()
    return [(n, d, A.pillow_pixels(d)) for n, d in A.pillow_cases(n=40)], A.refused_cases()


def mixed_batch(kind: str):
    """[(name, file, expected status, expected pixels or None)]: up to nine decodable files of different shapes from 1 x 1 to
    64 x 64 (tiffc: LZW and PackBits files alternating), two the parser leaves to Pillow (1), the kind's CUT cases (2) and an
    empty file, shuffled."""
    good, refused = _material(kind)
    by_shape = {}
    for name, data, px in good:
        if max(px.shape[:2]) <= 64:
            by_shape.setdefault(px.shape + (("packbits" in name, "_p2_" in name) if kind == "tiffc" else ()), (name, data, px))
    shapes = sorted(by_shape, key=lambda s: (s[0] * s[1], s))
    picked = [by_shape[s] for s in sorted(set(shapes[:: max(1, len(shapes) // 7)][:7] + [shapes[0], shapes[-1]]))]
    assert shapes[0][:2] == (1, 1) and len(picked) >= 4
    left = [r for r in refused if r[2] == 1][:2]
    cut = [r for r in refused if r[0] in CUT[kind]]
    assert len(left) == 2 and len(cut) == len(CUT[kind]) and all(r[2] == 2 for r in cut)
    batch = [(n, d, 0, px) for n, d, px in picked] + [(n, d, 1, None) for n, d, _ in left] + [(n, d, 2, None) for n, d, _ in cut]
    batch.append(("empty", b"", EMPTY[kind], None))
    order = np.random.default_rng(len(kind) * 31 + len(batch)).permutation(len(batch))
    return [batch[k] for k in order]


def _idat_bytes(png: bytes) -> int:
    """The bytes of a PNG file's zlib stream: the sum of its IDAT payloads."""
    pos, total = 8, 0
    while pos + 12 <= len(png):
        length = int.from_bytes(png[pos:pos + 4], "big")
        total += length if png[pos + 4:pos + 8] == b"IDAT" else 0
        pos += 12 + length
    return total


def sub_batches(kind: str, batch) -> list:
    """How many of the batch's decodable images each sub-batch of the decode call holds under BUDGET[kind]: the decoder's
    order and cost function written out again (ke_webp_frame_scratch, ke_vp8l_scratch_words, ke_webpa_plane_words; for tiffc
    a lower bound: every LZW image's dictionaries alone exceed the budget, and the PackBits images are counted as one)."""
    pad16 = lambda b: (b + 15) & ~15
    frame = lambda w, h: pad16(((w + 15) // 16) * ((h + 15) // 16) * 1172)
    vp8l = lambda w, h: pad16(4 * (2 * w * h + 3 * ((w + 3) // 4) * ((h + 3) // 4) + 19304))
    good = [(n, d, px.shape[1], px.shape[0]) for n, d, st, px in batch if st == 0]
    if kind == "png":
        # streams padded to 16 + the filtered rows (a filter byte each) and 32 bytes, padded + a copy record per 3 bytes and two
        zlen = {n: _idat_bytes(d) for n, d, _, _ in good}
        good.sort(key=lambda g: -zlen[g[0]])                              # stable, by the IDAT payloads' bytes
        raw = {n: px.shape[0] * (px.shape[1] * (px.shape[2] if px.ndim == 3 else 1) + 1) for n, _, st, px in batch if st == 0}
        costs = [pad16(zlen[n]) + pad16(raw[n] + 32) + 8 * (raw[n] // 3 + 2) for n, *_ in good]
    elif kind == "tiffc":
        lzw = sum("lzw" in n for n, *_ in good)
        return [1] * lzw + ([len(good) - lzw] if len(good) > lzw else [])
    elif kind == "webpa":
        good.sort(key=lambda g: -len(W.vp8_of(g[1])))                     # stable, by the frame's bytes
        plane = lambda d, w, h: 0 if A.header_byte(d) is None else vp8l(w, h) if A.header_byte(d) & 3 == 1 else pad16(4 * ((w * h + 3) // 4))
        costs = [frame(w, h) + plane(d, w, h) for _, d, w, h in good]
    else:
        good.sort(key=lambda g: -len(g[1]))                               # stable, by the file's bytes
        costs = [(frame if kind == "webp" else vp8l)(w, h) for _, _, w, h in good]
    counts, used = [], 0
    for c in costs:
        if counts and used + c <= BUDGET[kind][1]:
            counts[-1], used = counts[-1] + 1, used + c
        else:
            counts.append(1)
            used = c
    return counts


@pytest.mark.parametrize("kind", sorted(set(BUDGET) - {"jpeg"}))      # (jpeg: the same bounds in the GPU test, from the call's count)
def test_budgets_cut_the_mixed_batch_into_three_sub_batches_or_more(kind):
    counts = sub_batches(kind, mixed_batch(kind))
    print(kind, BUDGET[kind], counts)
    assert len(counts) >= 3 and max(counts) >= 2, counts           # the loop advances twice at least, and packs as well


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_batch_keeps_every_status_and_pixel_at_its_index(kind, monkeypatch):
    from kobato_eyes_amd import _native

    ctx = _native.get_context(0)
    batch = mixed_batch(kind)
    if kind in BUDGET:
        monkeypatch.setenv(BUDGET[kind][0], str(BUDGET[kind][1]))
    out, status = ctx.decode([d for _, d, _, _ in batch], kind)
    assert status.tolist() == [s for _, _, s, _ in batch], [n for n, *_ in batch]
    if kind in BUDGET:
        assert ctx.last_decode_sub_batches() >= 3, (kind, ctx.last_decode_sub_batches())
    if kind in ("jpeg", "png"):                                    # a condition on the inputs: some sub-batch packs two or more
        assert ctx.last_decode_sub_batches() < sum(s == 0 for _, _, s, _ in batch), (kind, ctx.last_decode_sub_batches())
    for k, (name, _, expected, px) in enumerate(batch):
        if expected == 0:
            assert out[k].shape == px.shape and np.array_equal(out[k], px), (kind, k, name)
        else:
            assert out[k] is None, (kind, k, name)


def _small_files(suffix: str):
    """Twelve files between 8 x 8 and 33 x 17, several of one shape so that groups form: PNG files (gray, RGB, RGBA), or .webp
    files (lossy, lossless, lossy with an alpha plane, and a lossy one cut in half)."""
    import io

    from PIL import Image

    rng = np.random.default_rng(len(suffix))
    sizes = [(8, 8), (33, 17), (8, 8), (17, 9)]
    files = []
    for k in range(12):
        w, h = sizes[k % 4]
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        alpha = rng.integers(0, 256, (h, w), dtype=np.uint8)
        if suffix == ".png":
            im = [Image.fromarray(a[..., 0]), Image.fromarray(a), Image.fromarray(np.dstack([a, alpha]), "RGBA")][k // 4]
            buf = io.BytesIO()
            im.save(buf, "PNG")
            files.append(buf.getvalue())
        else:
            files.append([W.pillow_file(a, 80, 4), L.pillow_file(Image.fromarray(a)), A.pillow_file(a, alpha)][k // 4])
    if suffix == ".webp":
        files[1] = files[1][: len(files[1]) // 2]
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("suffix,kinds", [(".png", ("png",)), (".webp", ("webp", "webpl", "webpa"))])
def test_bytes_paths_and_a_span_read_ahead_are_one_decode(suffix, kinds, tmp_path):
    """Context.hash of the same twelve files as bytes, as paths and as a span of a batch read ahead with two files skipped
    (five files of another batch lie before the span): the same (phash, dhash, status) at every file that was not skipped,
    status 1 at the two that were -- for a base kind and each of its follow-ups.  And decode_files_owned lays the same pixels
    out by shape and in 16-byte slots.  Every step has a time limit of its own: a call that hangs ends the run."""
    import faulthandler
    from contextlib import contextmanager

    from kobato_eyes_amd import _native

    @contextmanager
    def within(seconds):
        faulthandler.dump_traceback_later(seconds, exit=True)
        try:
            yield
        finally:
            faulthandler.cancel_dump_traceback_later()

    ctx = _native.get_context(0)
    files = _small_files(suffix)
    paths = []
    for k, data in enumerate(files):
        paths.append(str(tmp_path / f"f{k:02d}{suffix}"))
        open(paths[-1], "wb").write(data)
    skip = np.zeros(12, bool)
    skip[[0, 7]] = True
    taken = np.zeros(12, bool)
    for kind in kinds:
        with within(60):
            p, d, st = ctx.hash(files, kind=kind)
        assert set(st.tolist()) <= {0, 1, 2}
        taken |= st == 0
        with within(60):
            p2, d2, st2 = ctx.hash_files(paths, kind=kind)
        assert (p2.tolist(), d2.tolist(), st2.tolist()) == (p.tolist(), d.tolist(), st.tolist()), kind
        with within(60):
            held = ctx.read_files_ahead(paths[:5] + paths, [(kind, 5, 17)])
            try:
                assert held is not None and len(held) == 17 and (kind, 5, 17) in held.probed
                p3, d3, st3 = ctx.hash(None, kind=kind, ahead=(held, 5, 17), skip=skip)
            finally:
                held.release()
        assert st3[skip].tolist() == [1, 1], kind                              # left alone: as if refused
        assert (p3[~skip].tolist(), d3[~skip].tolist(), st3[~skip].tolist()) == (p[~skip].tolist(), d[~skip].tolist(), st[~skip].tolist()), kind
        with within(60):
            pixels = {}
            for by_shape in (False, True):
                dev, off, w, h, c, st4, flags = ctx.decode_files_owned(paths, kind, by_shape=by_shape)
                try:
                    assert st4.tolist() == st.tolist() and flags.shape == (12,)
                    for i in np.nonzero(st4 == 0)[0].tolist():
                        px = np.empty((h[i], w[i], c[i]), np.uint8)
                        ctx.memcpy(px, dev + int(off[i]), px.nbytes)
                        pixels.setdefault(i, []).append(px)
                    if by_shape:
                        assert (off[st4 != 0] == _native.NOT_LAID).all()
                        runs = _native.runs_laid_out(off, (w, h, c))
                        assert sorted(np.concatenate(runs).tolist()) == np.nonzero(st4 == 0)[0].tolist() and any(len(r) > 1 for r in runs)
                finally:
                    if dev:
                        ctx.free(dev)
            assert pixels and all(len(v) == 2 and np.array_equal(v[0], v[1]) for v in pixels.values()), kind
    if suffix == ".webp":
        assert taken.tolist() == [True, False] + [True] * 10     # every file but the cut one is somebody's
    else:
        assert taken.all()


def _jpeg_files_for_the_cut():
    """24 JPEG files, none larger than 64 x 64, shuffled: sequential ones of every sampling, progressive ones (five in a row and
    three apart in the caller's order), restart files written by hand (tests/_jpeg_rst_cases.py) and two of their deviants, a
    file cut at two thirds and one that is no JPEG."""
    import _jpeg_rst_cases as R

    rng = np.random.default_rng(24)
    image = lambda w, h: J._image(rng, w, h, 2)
    seq = [J._save(image(w, h), quality=85, subsampling=sub) for (w, h), sub in (((64, 64), 2), ((17, 33), 0), ((33, 17), 1), ((9, 9), 2), ((1, 1), 0))]
    seq += [J._save(image(40, 24)[:, :, 1], quality=80), J.with_luma_sampling(J._save(image(33, 40), quality=88, subsampling=1), 0x12)]
    prog = [J._save(image(w, h), quality=85, subsampling=sub, progressive=True)
            for (w, h), sub in (((64, 64), 0), ((17, 33), 2), ((8, 8), 1), ((5, 3), 0), ((48, 40), 2), ((31, 64), 1), ((2, 2), 0))]
    prog.append(J._save(image(24, 40)[:, :, 1], quality=80, progressive=True))
    by_name = dict(R.handwritten())
    rst = [by_name[n] for n in ("rst_gray_37x22_ri1_zeros", "rst_gray_37x22_ri7_ones", "rst_444_37x22_ri2_ones", "rst_444_37x22_ri16_zeros",
                                "rst_440_37x46_ri3_zeros")]
    dev = [d for n, d, *_ in R.deviants() if n in ("dev_wrong_number_on_marker_2", "dev_leftover_bytes_in_front_of_markers")]
    assert len(rst) == 5 and len(dev) == 2
    cut = J._save(J._image(rng, 64, 48, 0), quality=85)                  # noise: two thirds of the file end inside the scan
    others = seq + rst + dev + prog[5:] + [cut[: len(cut) * 2 // 3], b"\x89PNG\r\n\x1a\n" + bytes(64)]
    order = rng.permutation(len(others)).tolist()
    files = [others[k] for k in order[:6]] + prog[:5] + [others[k] for k in order[6:]]          # five progressive neighbours
    assert len(files) == 24
    return files


@pytest.mark.gpu
def test_jpeg_sub_batches_decode_what_one_sub_batch_decodes(monkeypatch):
    """The JPEG call with its scratch unbounded (one sub-batch) and bounded by 20 000 B (a 64 x 64 file alone takes more, two
    37 x 22 4:4:4 files of 8 640 B each fit, six gray ones of 2 880 B fit): the same statuses, pixels and split counts -- plain,
    with every restart file split into lanes of one MCU or more, at mixed scales, with both, and in the caller's order (where
    the progressive files of a sub-batch are several runs of neighbours, not one).  What one sub-batch decodes is held to Pillow
    by test_gpu_jpeg.py, test_gpu_jpeg_restarts.py and test_jpeg_scaled_cpu.py."""
    from kobato_eyes_amd import _native

    ctx = _native.get_context(0)
    files = _jpeg_files_for_the_cut()
    denoms = np.array([(1, 2, 4, 8)[k % 4] for k in range(len(files))], np.int32)
    split = {"KE_JPEG_SPLIT_RESTARTS": "1", "KE_JPEG_SPLIT_MIN_MCUS": "1"}
    for name, env, scaled in (("plain", {}, False), ("split", split, False), ("scaled", {}, True), ("split and scaled", split, True),
                              ("caller's order", {"KE_JPEG_KEEP_ORDER": "1"}, False)):
        for var in ("KE_JPEG_SCRATCH_BYTES", "KE_JPEG_SPLIT_RESTARTS", "KE_JPEG_SPLIT_MIN_MCUS", "KE_JPEG_KEEP_ORDER"):
            monkeypatch.delenv(var, raising=False)
        for var, value in env.items():
            monkeypatch.setenv(var, value)
        decode = (lambda: ctx.jpeg_decode_scaled(files, denoms)[:2]) if scaled else (lambda: ctx.decode(files, "jpeg"))
        whole, st_whole = decode()
        assert ctx.last_decode_sub_batches() == 1, name
        split_whole = ctx.jpeg_last_split()
        monkeypatch.setenv("KE_JPEG_SCRATCH_BYTES", "20000")
        parts, st_parts = decode()
        print(name, ctx.last_decode_sub_batches(), split_whole, st_whole.tolist())
        assert ctx.last_decode_sub_batches() >= 3, name
        assert ctx.jpeg_last_split() == split_whole and (split_whole[0] > 0) == bool(env.get("KE_JPEG_SPLIT_RESTARTS")), name
        assert st_parts.tolist() == st_whole.tolist() and sorted(set(st_whole.tolist())) == [0, 2], name
        assert sum(s == 0 for s in st_whole) >= 20, name
        for k, (a, b) in enumerate(zip(whole, parts)):
            assert (a is None and b is None and st_whole[k] != 0) or (a.shape == b.shape and np.array_equal(a, b)), (name, k)
