"""The tail of the single-pass hash kernels with its vertical taps on the matrix cores (fused_tail_mx, csrc/ke_hash.hip),
on an MI355X: every case against the CPU oracle bit for bit -- pHash, dHash, both tiles, tie margins -- and against the same
call with the dot-product tail (KE_VTILE_VALU=1), which must give the same bytes.

tests/conftest.py sets KE_FUSED_MIN_IMAGES=1, so the few images of a case run one workgroup per image and not band mode.
The shapes: both fixed-width instantiations of the benchmark's kernel; run-time row lengths; a row that does not end on a
quad; a single tile of fewer than 64 rows (128 x 7 is below the single-pass kernels' 16 rows and checks the path it falls
to); heights one past and one short of a 64-row operand step; 256 x 3000, which the single-pass kernels take per band only and which so holds
the banded finish to the same bytes, then the tallest 256-pixel rows that do run in one pass with this tail, for one hash
(1843 rows, 18 steps per block) and for both (1274 rows, 6 dHash steps per wave): the loops behind the first group of steps
(tests/test_fused_tail_plan_cpu.py holds those plans); 4-byte and 1-byte pixels; the 512-thread kernel with both hashes, at its first
and last instantiation, and with a width that is no multiple of 64."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = [
    # name, w, h, channels, images
    ("mx_256", 256, 256, 3, 6), ("mx_512", 512, 512, 3, 4),
    ("gen_68x40", 68, 40, 3, 8), ("gen_700x95", 700, 95, 3, 4),
    ("unal_70x33", 70, 33, 3, 8),
    ("rows_7", 128, 7, 3, 8), ("rows_31", 128, 31, 3, 8),
    ("rows_65", 256, 65, 3, 6), ("rows_127", 256, 127, 3, 6),
    ("rows_3000", 256, 3000, 3, 3), ("rows_1843", 256, 1843, 3, 3), ("rows_1274", 256, 1274, 3, 3),
    ("rgbx_512", 512, 512, 4, 3), ("l_512", 512, 512, 1, 4),
    ("wide_1024x64", 1024, 64, 3, 4), ("wide_2048x48", 2048, 48, 3, 4), ("wide_1100x40", 1100, 40, 3, 4),
]


@pytest.fixture(scope="module")
def ctx():
    from kobato_eyes_amd import _native

    return _native.get_context(0)  # raises loudly when the HIP library or the GPU is missing


def pixels(seed, n, w, h, c):
    rng = np.random.default_rng(seed)
    shape = (n, h, w) if c == 1 else (n, h, w, c)
    px = rng.integers(0, 256, shape, dtype=np.uint8)
    px[1] = (rng.integers(0, 2, shape[1:]) * 255).astype(np.uint8)      # clips on both sides
    px[2] = 255                                                         # every sum at its largest
    return px


def run(ctx, px, n, w, h, c):
    mg, mg_alone = np.empty(n, np.float32), np.empty(n, np.float32)
    ph, dh = ctx.hash_uniform(px, n, w, h, c, margin_out=mg)
    alone, _ = ctx.hash_uniform(px, n, w, h, c, want_dhash=False, margin_out=mg_alone)      # the kernels without a dHash leg
    t32, t98 = ctx.luma_tiles_uniform(px, n, w, h, c)
    t32_alone, _ = ctx.luma_tiles_uniform(px, n, w, h, c, want98=False)
    return {"phash": ph, "dhash": dh, "margin": mg, "phash_alone": alone, "margin_alone": mg_alone, "tile32": t32, "tile98": t98,
            "tile32_alone": t32_alone}


@pytest.mark.parametrize("name,w,h,c,n", CASES, ids=[case[0] for case in CASES])
def test_matrix_core_tail(ctx, monkeypatch, name, w, h, c, n):
    px = pixels(len(name) * 1000 + w + h, n, w, h, c)
    monkeypatch.delenv("KE_VTILE_VALU", raising=False)
    got = run(ctx, px, n, w, h, c)
    for k in range(n):
        ep, ed, e32, e98, em = O.hash_image(px[k], want_tiles=True)
        assert np.array_equal(got["tile32"][k], e32) and np.array_equal(got["tile32_alone"][k], e32), (name, k, "tile32")
        assert np.array_equal(got["tile98"][k], e98), (name, k, "tile98")
        assert int(got["phash"][k]) == ep and int(got["phash_alone"][k]) == ep, (name, k, "phash")
        assert int(got["dhash"][k]) == ed, (name, k, "dhash")
        assert got["margin"][k] == np.float32(em) and got["margin_alone"][k] == np.float32(em), (name, k, "margin")
    monkeypatch.setenv("KE_VTILE_VALU", "1")
    valu = run(ctx, px, n, w, h, c)
    for key in got:
        assert np.array_equal(got[key], valu[key]), (name, key, "the two tails differ")
