"""The GPU JPEG decoder (csrc/ke_jpeg.hip) behind its entropy decoder, on hand-written files (tests/_jpeg_sample_cases.py): what
only exists on the device -- ke_jpeg_idct's dequantisation, its 24-bit multiplies (IdctMul24) and the per-file status it writes
from many threads, upsample4_fast / chroma4 with their unclamped 4-byte loads, ycc_to_rgb24's v_mad_i32_i24 with the folded
offset -- on blocks within a few units of ke_idct_islow's bound on either side, on planes whose padding holds other values
than the last real column and row, and on every pair of two of (Y, Cb, Cr).  The judge is Pillow; the host build of the same
headers (tests/test_jpeg_cpu.py) must agree on every status.  No tolerances: pixels are equal or the test fails."""
from __future__ import annotations

import numpy as np
import pytest

import _jpeg_sample_cases as C
import test_jpeg_cpu as T
from oracle import oracle as O
from test_gpu_jpeg_streams import _equal, ctx, time_limit  # noqa: F401  (ctx: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def _first_difference(out, ref):
    if out is None or out.shape != ref.shape:
        return None if out is None else out.shape
    y, x, *ch = (int(v) for v in np.argwhere(out != ref)[0])
    return x, y, (ch[0] if ch else 0), int(out[(y, x) + tuple(ch)]), int(ref[(y, x) + tuple(ch)])


def test_blocks_on_either_side_of_the_idct_bound_in_one_shuffled_call(ctx):
    """All bound cases in ONE call, shuffled: statuses equal the host build's file by file; a file whose blocks are all inside
    the bound has Pillow's pixels, one with a block outside has status 1 and no pixels.  Then the taken files alone: all of
    them come back with status 0 (ke_jpeg_idct writes status[img] from many threads: it is per file and per call)."""
    cases = C.bound_cases()
    refs = C.references()
    blobs = [c[1] for c in cases]
    order = np.random.default_rng(81).permutation(len(blobs))
    with time_limit(60):
        out, status = ctx.jpeg_decode([blobs[k] for k in order])
    pixels, statuses = [None] * len(blobs), [None] * len(blobs)
    for at, k in enumerate(order):
        pixels[k], statuses[k] = out[at], int(status[at])
    L = T._lib()
    wrong = [(c[0], statuses[k]) for k, c in enumerate(cases) if statuses[k] != T._decode(L, c[1])[0]]
    assert not wrong, wrong[:20]
    wrong = [(c[0], statuses[k], _first_difference(pixels[k], refs[c[0]])) for k, c in enumerate(cases)
             if c[2].status == 0 and (statuses[k] != 0 or not _equal(pixels[k], refs[c[0]]))]
    assert not wrong, wrong[:20]
    wrong = [(c[0], statuses[k]) for k, c in enumerate(cases) if c[2].status == 1 and (statuses[k] != 1 or pixels[k] is not None)]
    assert not wrong, wrong[:20]
    taken = [c for c in cases if c[2].status == 0]
    assert len(taken) >= 300 and len(cases) - len(taken) >= 350
    with time_limit(60):
        out, status = ctx.jpeg_decode([c[1] for c in taken])
    wrong = [(c[0], int(status[k])) for k, c in enumerate(taken) if status[k] != 0 or not _equal(out[k], refs[c[0]])]
    assert not wrong, wrong[:20]


def _check_padding(ctx, cases):
    refs = C.references()
    with time_limit(60):
        out, status = ctx.jpeg_decode([c[1] for c in cases])
    wrong = [(c[2].sampling, c[2].size, int(status[k]), _first_difference(out[k], refs[c[0]])) for k, c in enumerate(cases)
             if status[k] != 0 or not _equal(out[k], refs[c[0]])]
    assert not wrong, wrong[:20]                                    # (sampling, size, status, (x, y, channel, got, Pillow's))


def test_planes_with_foreign_padding_in_one_call_of_mixed_sizes(ctx):
    """Every padding case in one call: ke_jpeg_colour's grid is sized by the call's largest width and height, so the small
    files meet its early exits next to the 515-wide ones."""
    cases = C.padding_cases()
    assert len(cases) >= 900 and max(c[2].size[0] for c in cases) == 515 and min(c[2].size for c in cases) == (1, 1)
    _check_padding(ctx, cases)


def test_planes_with_foreign_padding_509_to_515_columns_wide(ctx):
    """... and the widest files in a call of their own: two and three 256-column workgroups, the npx < 4 tail."""
    cases = [c for c in C.padding_cases() if c[2].size[0] >= 509]
    assert {c[2].size for c in cases} == {(w, h) for w in (509, 513, 515) for h in (31, 33, 63, 65, 66)}
    _check_padding(ctx, cases)


def test_every_pair_of_two_of_y_cb_cr(ctx):
    cases = C.colour_cases()
    refs = C.references()
    with time_limit(60):
        out, status = ctx.jpeg_decode([c[1] for c in cases])
    for k, (name, data, facts) in enumerate(cases):
        assert status[k] == 0 and out[k] is not None and out[k].shape == refs[name].shape, name
        if not np.array_equal(out[k], refs[name]):
            y, x, ch = (int(v) for v in np.argwhere(out[k] != refs[name])[0])
            triple = tuple(int(v) for v in C.ycc(data)[y, x])
            pytest.fail(f"{name}: (Y, Cb, Cr) = {triple} at ({x}, {y}) gives {out[k][y, x].tolist()}, Pillow {refs[name][y, x].tolist()} (channel {ch})")


def test_bound_and_padding_files_through_decode_and_hash(ctx):
    """The taken bound files and the 17 x 17 padding files through the decode -> hash seam of the batch hasher, in one call:
    the hashes are the oracle's of Pillow's pixels."""
    refs = C.references()
    cases = [c for c in C.bound_cases() if c[2].status == 0 and min(c[2].size) >= 16] + [c for c in C.padding_cases() if c[2].size == (17, 17)]
    assert sum(c[0].startswith("padding") for c in cases) >= 3 and len(cases) >= 300
    with time_limit(60):
        ph, dh, status = ctx.jpeg_hash([c[1] for c in cases])
    wrong = [c[0] for k, c in enumerate(cases) if status[k] != 0 or (int(ph[k]), int(dh[k])) != O.hash_image(refs[c[0]])]
    assert not wrong, wrong[:20]
