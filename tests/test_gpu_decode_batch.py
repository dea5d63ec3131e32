"""The host side the nine GPU decoders share (csrc/ke_decode_batch.h): accept, sort, pack into sub-batches, scatter the statuses.
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
# 77 KB and more, an LZW strip's dictionaries 2 MB (such an image is a sub-batch of its own; the PackBits files pack together)
BUDGET = {"webp": ("KE_WEBP_SCRATCH_BYTES", 6000), "webpl": ("KE_WEBP_SCRATCH_BYTES", 250000),
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


def sub_batches(kind: str, batch) -> list:
    """How many of the batch's decodable images each sub-batch of the decode call holds under BUDGET[kind]: the decoder's
    order and cost function written out again (ke_webp_frame_scratch, ke_vp8l_scratch_words, ke_webpa_plane_words; for tiffc
    a lower bound: every LZW image's dictionaries alone exceed the budget, and the PackBits images are counted as one)."""
    pad16 = lambda b: (b + 15) & ~15
    frame = lambda w, h: pad16(((w + 15) // 16) * ((h + 15) // 16) * 1172)
    vp8l = lambda w, h: pad16(4 * (2 * w * h + 3 * ((w + 3) // 4) * ((h + 3) // 4) + 19304))
    good = [(n, d, px.shape[1], px.shape[0]) for n, d, st, px in batch if st == 0]
    if kind == "tiffc":
        lzw = sum("lzw" in n for n, *_ in good)
        return [1] * lzw + ([len(good) - lzw] if len(good) > lzw else [])
    if kind == "webpa":
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


@pytest.mark.parametrize("kind", sorted(BUDGET))
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
    for k, (name, _, expected, px) in enumerate(batch):
        if expected == 0:
            assert out[k].shape == px.shape and np.array_equal(out[k], px), (kind, k, name)
        else:
            assert out[k] is None, (kind, k, name)
