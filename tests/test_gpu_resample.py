"""The general resampler (csrc/ke_hash.hip: ke_launch_resize_group -> resample_banded / resample_generic) against Pillow itself,
byte for byte, at every branch of the plan it launches, and ke_tile_ahash / ke_sad_pairs against their definitions in integers.

The plan depends on the shape: chunks of 8..32 dwords, 1..32 of them per output, one or several horizontal launches, one or
several row bands, the dword or the funnel-shift loader, vertical taps on the matrix cores or the VALU, and five reasons to fall
back to the generic passes.  ROWS steers it; ke_last_resize_plan (Context.last_resize_plan) says what the device ran, and the
coverage test holds the rows to the branches they are there for.  The reference is
Image.fromarray(px, mode).convert("L").resize((ow, oh), FILTER) for modes L, RGB and RGBX; there is no tolerance."""
from __future__ import annotations

import faulthandler
import time
from contextlib import contextmanager

import numpy as np
import pytest
from PIL import Image, ImageOps

from oracle import oracle as O

pytestmark = pytest.mark.gpu

LANCZOS, BILINEAR, BICUBIC = 0, 1, 2                                     # include/keyes.h KE_FILTER_*
PIL_FILTER = {LANCZOS: Image.LANCZOS, BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC}
MODE = {1: "L", 3: "RGB", 4: "RGBX"}
BANDED, CPO, NDWC, LAUNCHES, BANDS, FUNNEL, VMX, VFIRST = range(8)       # entries of ke_last_resize_plan


_state = {"device_suspect": None}      # set when a call came back with a HIP error: nothing more is started on the card


@contextmanager
def time_limit(seconds: int = 60):
    """A time limit of its own around one GPU step: a call that hangs in native code ends the whole run (a Python exception
    could not interrupt it), and after a HIP error no further step starts."""
    if _state["device_suspect"]:
        pytest.fail(f"not started: {_state['device_suspect']}")
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    except RuntimeError as exc:
        _state["device_suspect"] = str(exc)
        raise
    finally:
        faulthandler.cancel_dump_traceback_later()


class Row:
    """One source shape, its targets, and the branch it is there for: `filt` is the filter the branch was worked out for
    (every row still runs all three), `channels` the channel counts it runs with, `banded` what entry [0] of the plan must be
    for `filt` at every target (a tuple: per target) -- for every filter where `any_filter` says that the reason does not
    depend on the taps."""

    filters = (LANCZOS, BILINEAR, BICUBIC)

    def __init__(self, name, w, h, n, targets, filt, banded=1, channels=(1, 3, 4), any_filter=False):
        self.name, self.w, self.h, self.n, self.targets, self.filt, self.channels, self.any_filter = name, w, h, n, targets, filt, channels, any_filter
        self.banded = banded if isinstance(banded, tuple) else (banded,) * len(targets)


# Batches hold at least three images (noise, then flat 255 and flat 0), so the single-image shapes run with n = 3.
ROWS = [
    Row("up_both", 64, 64, 3, [(100, 90)], BICUBIC),                     # upscale both axes, ndwc 8, 6 vertical MFMA tiles
    Row("up_down", 100, 64, 3, [(64, 100)], LANCZOS),                    # one axis up, one down
    Row("identity_axis", 300, 200, 3, [(300, 77), (77, 200)], BICUBIC),  # identity axis on either side; 2 launches at cpo 1
    Row("ndwc16", 640, 96, 3, [(128, 33)], LANCZOS),                     # ndwc 16, 2 bands, oh across a 16-row tile
    Row("funnel_valu", 641, 97, 3, [(129, 129)], BILINEAR),              # funnel loader (w % 4 != 0), oh = 129 -> VALU vertical
    Row("launch_of_one", 600, 300, 3, [(257, 128), (300, 129)], LANCZOS),  # second launch with one output; oh 128 / 129
    Row("ndw32", 2340, 24, 3, [(130, 12), (128, 12)], LANCZOS, channels=(1,)),   # ndwc 32 at cpo 1 against cpo 2 x ndwc 16
    Row("cpo2_funnel", 1170, 24, 3, [(64, 24)], LANCZOS, channels=(3,)),  # cpo 2 with the funnel loader
    Row("ndwc24", 3000, 40, 3, [(300, 40)], LANCZOS),                    # ndwc 24, 2 launches, identity vertical
    Row("cpo16_l", 4096, 40, 3, [(16, 17)], LANCZOS),                    # cpo 16, ndwc 24, oh 17
    Row("cpo16_c", 4096, 40, 3, [(16, 16)], BICUBIC),                    # cpo 16, ndwc 16, oh 16
    Row("cpo32", 8192, 8, 3, [(12, 8)], BICUBIC, channels=(1,)),         # cpo 32, ndwc 24, 2 launches of 8 outputs
    Row("cpo32_funnel", 8190, 8, 3, [(13, 8)], LANCZOS, channels=(3,)),  # cpo 32, ndwc 32, funnel
    Row("window_too_long", 8192, 8, 3, [(12, 8)], LANCZOS, banded=0, channels=(1,)),   # window of 1028 dwords -> generic
    Row("row_too_long", 8196, 8, 3, [(64, 8)], BILINEAR, banded=0, channels=(1,), any_filter=True),   # row over 2048 quads -> generic
    Row("lds_too_large", 16, 600, 3, [(64, 64)], BILINEAR, banded=0, channels=(1,)),   # LDS over 64 KiB -> generic
    Row("lds_fits", 16, 200, 3, [(64, 64)], BILINEAR, channels=(1,)),    # ... and the same columns, shorter, stay banded
    Row("mfma_63_steps", 40, 4000, 3, [(20, 16)], LANCZOS, channels=(1,)),   # 63 MFMA steps per tile
    Row("vertical_first", 40, 4001, 3, [(20, 16)], LANCZOS, banded=0, channels=(1,), any_filter=True),   # one row more -> vertical-first generic
    Row("px_1x3", 1, 3, 3, [(4, 4)], LANCZOS, banded=0, channels=(1,), any_filter=True),   # under 4 pixels -> generic
    Row("px_3x1", 3, 1, 3, [(4, 4)], LANCZOS, banded=0, channels=(1,), any_filter=True),
    Row("px_1x1", 1, 1, 3, [(4, 4)], LANCZOS, banded=0, channels=(1,), any_filter=True),
    Row("smallest_banded", 2, 2, 3, [(5, 5)], LANCZOS),                  # the smallest banded image
    Row("n3", 64, 200, 3, [(48, 50)], BILINEAR, channels=(1,)),
    Row("n1500", 64, 200, 1500, [(48, 50)], BILINEAR, channels=(1,)),   # image index arithmetic at large n
    Row("bands4", 64, 2000, 3, [(48, 127)], LANCZOS, channels=(1,)),     # 4 bands, 8 MFMA tiles
    Row("bands32", 200, 5000, 3, [(100, 300)], LANCZOS, channels=(1,)),  # 32 bands, VALU vertical, 9 of 100 columns per group
    # column clamp and tile edges of ke_vtile_mx
    Row("tile_edges", 96, 80, 3, [(ow, oh) for ow in (15, 16, 17) for oh in (15, 16, 17, 31, 32, 33)], BILINEAR),
]
ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS)


def make_pixels(row: Row, ch: int) -> np.ndarray:
    """Seeded noise; the last two images of the batch are flat 255 and flat 0."""
    seed = [r.name for r in ROWS].index(row.name) * 8 + ch
    px = np.random.default_rng(seed).integers(0, 256, (row.n, row.h, row.w, ch), dtype=np.uint8)
    px[-2], px[-1] = 255, 0
    return px[..., 0].copy() if ch == 1 else px


_luma, _want = {}, {}


def pillow_luma(row: Row, ch: int) -> list:
    key = (row.name, ch)
    if key not in _luma:
        px = make_pixels(row, ch)
        _luma[key] = [Image.fromarray(px[k], MODE[ch]).convert("L") for k in range(row.n)]
    return _luma[key]


def pillow_resize(row: Row, ch: int, ow: int, oh: int, filt: int) -> np.ndarray:
    """The reference, computed once per case and shared by the tests."""
    key = (row.name, ch, ow, oh, filt)
    if key not in _want:
        out = np.stack([np.asarray(im.resize((ow, oh), PIL_FILTER[filt])) for im in pillow_luma(row, ch)])
        out.setflags(write=False)
        _want[key] = out
    return _want[key]


def cases(row: Row):
    return [(ch, ow, oh, f) for ch in row.channels for (ow, oh) in row.targets for f in row.filters]


@pytest.fixture(scope="module")
def ctx():
    from kobato_eyes_amd import _native

    with time_limit():
        return _native.get_context(0)


_ran = {}


def run_row(ctx, row: Row) -> dict:
    """{(ch, ow, oh, filter): (thumbnails, plan)} of a row, each call under its own time limit; run once per module."""
    if row.name not in _ran:
        got = {}
        for ch in row.channels:
            px = make_pixels(row, ch)
            for (c, ow, oh, f) in cases(row):
                if c != ch:
                    continue
                with time_limit():
                    out = ctx.resize_luma_uniform(px, row.n, row.w, row.h, ch, ow, oh, f)
                    got[(ch, ow, oh, f)] = (out, ctx.last_resize_plan())
        _ran[row.name] = got
    return _ran[row.name]


def differing(row: Row, got: dict) -> list:
    bad = []
    for (ch, ow, oh, f), (out, plan) in got.items():
        want = pillow_resize(row, ch, ow, oh, f)
        if out.shape != want.shape or not np.array_equal(out, want):
            diff = np.argwhere(out != want) if out.shape == want.shape else []
            bad.append((row.name, ch, (ow, oh), f, plan, len(diff), [tuple(int(v) for v in d) for d in diff[:3]]))
    return bad


def test_a_null_context_is_refused_and_a_fresh_one_reports_nothing():
    from kobato_eyes_amd import _native

    lib = _native.load_library()
    plan = np.zeros(8, np.int32)
    assert lib.ke_last_resize_plan(None, plan.ctypes.data) == -1           # KE_EINVAL
    with time_limit():
        fresh = _native.Context(0)
        try:
            assert fresh.last_resize_plan() == (-1,) * 8
            with pytest.raises(ValueError):
                fresh._check(lib.ke_last_resize_plan(fresh._h, None), "ke_last_resize_plan")
        finally:
            fresh.close()


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_row_equals_pillow_and_takes_its_branch(ctx, name):
    row = ROW[name]
    got = run_row(ctx, row)
    assert len(got) == len(cases(row))
    for key, (out, plan) in got.items():
        print(name, key, plan)
    assert not differing(row, got)
    for (ch, ow, oh, f), (_, plan) in got.items():
        # the shape of a report, whatever the branch: entries that do not apply are -1
        if plan[BANDED] == 1:
            assert plan[VFIRST] == -1 and min(plan[CPO:VFIRST]) >= 0, (name, ch, ow, oh, f, plan)
            assert plan[CPO] in (1, 2, 4, 8, 16, 32) and plan[NDWC] in (8, 16, 24, 32) and plan[LAUNCHES] >= 1 and plan[BANDS] >= 1
            assert plan[LAUNCHES] == -(-ow // min(ow, 256 // plan[CPO])), (name, ch, ow, oh, f, plan)   # 256 lanes per launch
            assert plan[FUNNEL] == (1 if row.w % 4 else 0) and plan[VMX] == (1 if oh <= 128 else 0), (name, ch, ow, oh, f, plan)
        else:
            assert plan[BANDED] == 0 and plan[CPO:VFIRST] == (-1,) * 6, (name, ch, ow, oh, f, plan)
            assert plan[VFIRST] == (1 if row.h > 100 * row.w and oh < row.h else 0), (name, ch, ow, oh, f, plan)
        if f == row.filt or row.any_filter:
            assert plan[BANDED] == row.banded[row.targets.index((ow, oh))], (name, ch, ow, oh, f, plan)


def test_the_rows_cover_every_branch_of_the_plan(ctx):
    """A condition on the rows, not a measurement: what ke_last_resize_plan reported over the whole grid."""
    plans = [plan for row in ROWS for (_, plan) in run_row(ctx, row).values()]
    banded = [p for p in plans if p[BANDED] == 1]
    generic = [p for p in plans if p[BANDED] == 0]
    assert len(banded) + len(generic) == len(plans)
    assert {p[NDWC] for p in banded} == {8, 16, 24, 32}
    assert {1, 2, 16, 32} <= {p[CPO] for p in banded}
    assert any(p[LAUNCHES] > 1 and p[CPO] == 1 for p in banded) and any(p[LAUNCHES] > 1 and p[CPO] > 1 for p in banded)
    assert any(p[BANDS] == 1 for p in banded) and any(p[BANDS] > 1 for p in banded)
    assert {p[FUNNEL] for p in banded} == {0, 1}
    assert {p[VMX] for p in banded} == {0, 1}
    assert {p[VFIRST] for p in generic} == {0, 1}
    # the rows named for a branch took it, for the filter the branch was worked out for
    took = {(r.name, t): run_row(ctx, r)[(r.channels[0], t[0], t[1], r.filt)][1] for r in ROWS for t in r.targets}
    assert took[("ndwc16", (128, 33))][NDWC] == 16 and took[("ndwc16", (128, 33))][BANDS] == 2
    assert took[("identity_axis", (300, 77))][LAUNCHES] == 2 and took[("launch_of_one", (257, 128))][LAUNCHES] == 2
    assert took[("ndw32", (130, 12))][CPO:LAUNCHES] == (1, 32) and took[("ndw32", (128, 12))][CPO:LAUNCHES] == (2, 16)
    assert took[("cpo2_funnel", (64, 24))][CPO] == 2 and took[("cpo2_funnel", (64, 24))][FUNNEL] == 1
    assert took[("ndwc24", (300, 40))][NDWC:BANDS] == (24, 2)
    assert took[("cpo16_l", (16, 17))][CPO:LAUNCHES] == (16, 24) and took[("cpo16_c", (16, 16))][CPO:LAUNCHES] == (16, 16)
    assert took[("cpo32", (12, 8))][CPO:BANDS] == (32, 24, 2) and took[("cpo32_funnel", (13, 8))][CPO:BANDS] == (32, 32, 2)
    assert took[("cpo32_funnel", (13, 8))][FUNNEL] == 1
    assert took[("bands4", (48, 127))][BANDS] == 4 and took[("bands32", (100, 300))][BANDS] == 32
    assert took[("vertical_first", (20, 16))][VFIRST] == 1 and took[("mfma_63_steps", (20, 16))][VMX] == 1


def test_the_valu_vertical_kernel_gives_the_same_bytes(ctx, monkeypatch):
    """KE_VTILE_VALU=1 takes the vertical taps of every banded shape on the VALU: every case with oh <= 128 that ran banded
    again, the 1500-image batch among them (ke_vtile takes one workgroup per image)."""
    first = {r.name: run_row(ctx, r) for r in ROWS}
    expected = sum(1 for got in first.values() for (_, _, oh, _), (_, plan) in got.items() if oh <= 128 and plan[BANDED] == 1)
    monkeypatch.setenv("KE_VTILE_VALU", "1")
    reran = 0
    for row in ROWS:
        for ch in row.channels:
            px = make_pixels(row, ch)
            for (c, ow, oh, f) in cases(row):
                before, plan_before = first[row.name][(c, ow, oh, f)]
                if c != ch or oh > 128 or plan_before[BANDED] != 1:
                    continue
                with time_limit():
                    out = ctx.resize_luma_uniform(px, row.n, row.w, row.h, ch, ow, oh, f)
                    plan = ctx.last_resize_plan()
                assert plan_before[VMX] == 1 and plan[VMX] == 0 and plan[:VMX] == plan_before[:VMX], (row.name, ch, ow, oh, f, plan, plan_before)
                assert np.array_equal(out, before), (row.name, ch, ow, oh, f)
                assert np.array_equal(out, pillow_resize(row, ch, ow, oh, f)), (row.name, ch, ow, oh, f)
                reran += 1
    # 162 at the tile edges, 9 for each of the nine three-channel targets with oh <= 128, 31 on the one-channel rows
    assert reran == expected == 274, (reran, expected)


@pytest.mark.parametrize("name,ch", [("launch_of_one", 3), ("cpo32", 1), ("vertical_first", 1)])
def test_device_resident_input_and_output(ctx, name, ch):
    row = ROW[name]
    px = make_pixels(row, ch)
    for (ow, oh) in row.targets:
        out = np.empty((row.n, oh, ow), np.uint8)
        with time_limit():
            d_in, d_out = ctx.malloc(px.nbytes), ctx.malloc(out.nbytes)
            try:
                ctx.memcpy(d_in, px, px.nbytes)
                ctx.resize_luma_uniform(d_in, row.n, row.w, row.h, ch, ow, oh, row.filt, out=d_out)
                plan = ctx.last_resize_plan()
                ctx.memcpy(out, d_out, out.nbytes)
            finally:
                ctx.free(d_in)
                ctx.free(d_out)
        host_out, host_plan = run_row(ctx, row)[(ch, ow, oh, row.filt)]
        assert plan == host_plan
        assert np.array_equal(out, host_out)
        assert np.array_equal(out, pillow_resize(row, ch, ow, oh, row.filt))


@pytest.mark.parametrize("name", ["up_both", "up_down", "ndwc16", "funnel_valu", "launch_of_one"])
def test_the_crop_box_of_fit_with_lanczos_and_bilinear(ctx, name):
    """ke_fit_luma_uniform with filters 0 and 1 (the SSIM step uses 2) on rows whose target has another aspect than the source:
    ImageOps.fit crops to the aspect, and the crop reaches the resampler as a fractional box."""
    row = ROW[name]
    ow, oh = row.targets[0]
    assert ow * row.h != oh * row.w
    for ch in (1, 3):
        px = make_pixels(row, ch)
        for f in (LANCZOS, BILINEAR):
            with time_limit():
                out = ctx.fit_luma_uniform(px, row.n, row.w, row.h, ch, ow, oh, f)
                plan = ctx.last_resize_plan()
            want = np.stack([np.asarray(ImageOps.fit(im, (ow, oh), PIL_FILTER[f])) for im in pillow_luma(row, ch)])
            print(name, ch, f, plan)
            assert np.array_equal(out, want), (name, ch, f, plan, int((out != want).sum()))


@pytest.mark.parametrize("box_first", [False, True])
def test_the_table_cache_keeps_a_boxed_axis_apart_from_the_whole_one(ctx, box_first):
    """The same (in, out, filter) with and without a source interval, back to back, in both orders: fit crops the 102 (106)
    columns to the middle 66 (70) and resizes them to 66 (70) outputs, resize maps all of them onto as many.  Sizes no other
    test uses, so neither table is cached before."""
    w, h, side = (106, 70, 70) if box_first else (102, 66, 66)
    px = np.random.default_rng(w).integers(0, 256, (3, h, w), dtype=np.uint8)
    ims = [Image.fromarray(p) for p in px]
    for f in (LANCZOS, BILINEAR, BICUBIC):
        calls = [("resize", lambda: ctx.resize_luma_uniform(px, 3, w, h, 1, side, side, f),
                  lambda: [im.resize((side, side), PIL_FILTER[f]) for im in ims]),
                 ("fit", lambda: ctx.fit_luma_uniform(px, 3, w, h, 1, side, side, f),
                  lambda: [ImageOps.fit(im, (side, side), PIL_FILTER[f]) for im in ims])]
        for what, run, ref in (calls[::-1] if box_first else calls) * 2:
            with time_limit():
                out = run()
            assert np.array_equal(out, np.stack([np.asarray(im) for im in ref()])), (what, f, box_first)


def test_results_survive_the_turnover_of_the_table_cache():
    """More axes than the cache keeps (2048 tables; beyond that the next call frees every one): 4-row gray images of widths
    8..1040 to 7 x 4, LANCZOS and then BILINEAR -- 2066 horizontal tables and two identity ones -- on a context of its own,
    every result against Pillow, and the first 20 widths again afterwards, against Pillow and against what they gave before."""
    from kobato_eyes_amd import _native

    widths = list(range(8, 1041))
    rng = np.random.default_rng(2048)
    images = {w: rng.integers(0, 256, (1, 4, w), dtype=np.uint8) for w in widths}
    want = {(w, f): np.asarray(Image.fromarray(images[w][0]).resize((7, 4), PIL_FILTER[f])) for f in (LANCZOS, BILINEAR) for w in widths}
    assert 2 * len(widths) > 2048
    with time_limit(120):
        own = _native.Context(0)
        try:
            t0 = time.perf_counter()
            kept, bad = {}, []
            for f in (LANCZOS, BILINEAR):
                for w in widths:
                    out = own.resize_luma_uniform(images[w], 1, w, 4, 1, 7, 4, f)[0]
                    if not np.array_equal(out, want[(w, f)]):
                        bad.append((w, f))
                    if w < 28:
                        kept[(w, f)] = out
            assert not bad, bad[:20]
            assert len(kept) == 40
            for (w, f), before in kept.items():
                out = own.resize_luma_uniform(images[w], 1, w, 4, 1, 7, 4, f)[0]
                assert np.array_equal(out, before) and np.array_equal(out, want[(w, f)]), (w, f)
            print(f"cache turnover: {2 * len(widths) + len(kept)} calls in {time.perf_counter() - t0:.2f} s")
        finally:
            own.close()


# ---- ke_tile_ahash and ke_sad_pairs against their definitions in integers -------------------------------------------------

GRIDS = [(1, 1), (1, 8), (3, 5), (4, 8), (8, 4), (17, 3), (64, 1), (64, 16), (1, 1024)]


def ahash_by_definition(thumbs: np.ndarray, grid: int, tile: int) -> np.ndarray:
    """Bit i, in order (gy, gx, ty, tx), is px * tile^2 > sum(tile); little-endian into ceil(side^2 / 64) words."""
    n, side = len(thumbs), grid * tile
    t = thumbs.reshape(n, grid, tile, grid, tile).transpose(0, 1, 3, 2, 4).astype(np.int64)
    bits = (t * (tile * tile) > t.sum(axis=(3, 4), keepdims=True)).reshape(n, side * side)
    words = (side * side + 63) // 64
    padded = np.zeros((n, words * 64), np.uint8)
    padded[:, :side * side] = bits
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(n, words)


@pytest.mark.parametrize("grid,tile", GRIDS)
def test_tile_ahash_is_its_definition(ctx, grid, tile):
    side = grid * tile
    rng = np.random.default_rng(grid * 2048 + tile)
    thumbs = np.empty((3, side, side), np.uint8)
    thumbs[0] = rng.integers(0, 256, (side, side))
    thumbs[1] = 255
    # every tile: tile^2 - 1 pixels of 100 and one of 101, at a place of its own
    one = np.full((grid, grid, tile * tile), 100, np.uint8)
    np.put_along_axis(one, rng.integers(0, tile * tile, (grid, grid, 1)), 101, axis=2)
    thumbs[2] = one.reshape(grid, grid, tile, tile).transpose(0, 2, 1, 3).reshape(side, side)
    want = ahash_by_definition(thumbs, grid, tile)
    for k in range(3):
        assert int.from_bytes(want[k].tobytes(), "little") == O.tile_ahash_bits(thumbs[k], grid, tile), k
    with time_limit():
        got = ctx.tile_ahash(thumbs, 3, grid, tile)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not got[1].any()                                              # flat: no pixel exceeds its tile's mean
    ones = sum(bin(int(v)).count("1") for v in got[2])
    assert ones == (grid * grid if tile > 1 else 0)                      # a tile of one pixel never exceeds itself


@pytest.mark.parametrize("grid,tile", [(0, 4), (65, 1), (33, 32)])
def test_tile_ahash_refuses_grids_beyond_its_limits(ctx, grid, tile):
    with pytest.raises(ValueError), time_limit():
        ctx.tile_ahash(np.zeros((1, max(grid * tile, 1), max(grid * tile, 1)), np.uint8), 1, grid, tile)


def sad_by_definition(thumbs, pa, pb):
    return np.array([np.abs(thumbs[a].astype(np.int64) - thumbs[b]).sum() for a, b in zip(pa, pb)], np.uint64)


@pytest.mark.parametrize("pixels", [1, 255, 256, 257, 4096, 1048576])
def test_sad_pairs_is_the_sum_of_absolute_differences(ctx, pixels):
    thumbs = np.random.default_rng(pixels).integers(0, 256, (4, pixels), dtype=np.uint8)
    thumbs[2], thumbs[3] = 255, 0
    pa, pb = [0, 1, 0, 1, 2, 3, 2, 3, 0], [0, 1, 1, 0, 3, 2, 2, 3, 2]
    with time_limit():
        got = ctx.sad_pairs(thumbs, 4, pixels, pa, pb)
    assert got.dtype == np.uint64 and np.array_equal(got, sad_by_definition(thumbs, pa, pb))
    assert not got[[0, 1, 6, 7]].any()                                   # (i, i)
    assert int(got[4]) == int(got[5]) == 255 * pixels                    # 267 386 880 at 2^20 pixels: beyond float32's integers


def test_sad_pairs_many_pairs_with_repeats_and_the_edges_of_the_call(ctx):
    pixels, n = 4096, 7
    rng = np.random.default_rng(300)
    thumbs = rng.integers(0, 256, (n, pixels), dtype=np.uint8)
    pa, pb = rng.integers(0, n, 300), rng.integers(0, n, 300)
    pa[100:110], pb[100:110] = pa[0], pb[0]                               # the same pair ten times over
    with time_limit():
        got = ctx.sad_pairs(thumbs, n, pixels, pa, pb)
    assert np.array_equal(got, sad_by_definition(thumbs, pa, pb))
    for a, b in [(n, 0), (0, n), (-1, 0), (0, -1)]:
        with pytest.raises(ValueError), time_limit():
            ctx.sad_pairs(thumbs, n, pixels, [0, a], [0, b])
    with time_limit():
        empty = ctx.sad_pairs(thumbs, n, pixels, [], [])
    assert empty.shape == (0,) and empty.dtype == np.uint64
