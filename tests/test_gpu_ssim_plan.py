"""The SSIM kernels (csrc/ke_ssim.hip: ke_ssim_waves, ke_ssim_fast) against the oracle at every branch of the launch plan
(csrc/ke_ssim_plan.h): both kernels x 1, 3 or 4 channels x 4 or 8 pixels per lane x the aligned or the funnel-shift loader x one
or several column blocks, the three reasons for not aligning, one or several row bands, band heights of 14 .. 126 rows, partial
last groups and bands, images at a misaligned device address, pairs that share a workgroup, and the NaN fill.

tests/_ssim_plan_cases.py holds the rows and builds their inputs, whose SSIM map steps at every seam between blocks and bands
(tests/test_ssim_plan_cases_cpu.py shows that one wrong window there moves a score by four times its bar or more).  Every row is
scored through ssim_pairs_uniform in both modes and held to O.ssim_luma(O.luma(a), O.luma(b)) at the bars of
tests/test_gpu_parity.py: 1e-6 for the exact kernel, 1e-5 for the fast one; the two modes lie within 1e-5 of each other.
ke_last_ssim_plan (Context.last_ssim_plan) says what the device ran, and the coverage test holds the rows to the branches they are
there for."""
from __future__ import annotations

import faulthandler
from contextlib import contextmanager

import numpy as np
import pytest

import _ssim_plan_cases as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def ctx():
    from kobato_eyes_amd import _native

    with time_limit():
        return _native.get_context(0)


def score(ctx, row: S.Row, px: np.ndarray, pa, pb, exact: bool):
    """(scores, plan) of one launch in one mode; the mode is put back whatever happens.  A row with a base offset has its images
    copied into device memory that many bytes past the start of an allocation, and hands that address over."""
    n = len(px)
    dev = None
    with time_limit():
        ctx.ssim_set_mode(exact)
        try:
            if row.base:
                dev = ctx.malloc(px.nbytes + 16)            # (the funnel-shift loader reads whole dwords: up to 3 bytes past the last image)
                ctx.memcpy(dev + row.base, np.ascontiguousarray(px), px.nbytes)
            got = ctx.ssim_pairs_uniform(dev + row.base if row.base else px, n, row.w, row.h, row.channels, pa, pb)
            return got, ctx.last_ssim_plan()
        finally:
            ctx.ssim_set_mode(False)
            if dev is not None:
                ctx.free(dev)


_ran = {}


def run_row(ctx, row: S.Row) -> dict:
    """A row scored in both modes, and the oracle's score of each of its distinct pairs; run once per module."""
    if row.name not in _ran:
        px = S.pixels(row)
        k = np.arange(row.pairs) % row.distinct
        out = {"want": np.array([O.ssim_luma(O.luma(px[2 * j]), O.luma(px[2 * j + 1])) for j in range(row.distinct)]), "which": k}
        for exact in (False, True):
            out[exact] = score(ctx, row, px, 2 * k, 2 * k + 1, exact)
        _ran[row.name] = out
    return _ran[row.name]


def test_a_null_context_is_refused_and_a_fresh_one_reports_nothing():
    from kobato_eyes_amd import _native

    lib = _native.load_library()
    plan = np.zeros(8, np.int32)
    assert lib.ke_last_ssim_plan(None, plan.ctypes.data) == -1             # KE_EINVAL
    with time_limit():
        fresh = _native.Context(0)
        try:
            assert fresh.last_ssim_plan() == (-1,) * 8
            with pytest.raises(ValueError):
                fresh._check(lib.ke_last_ssim_plan(fresh._h, None), "ke_last_ssim_plan")
        finally:
            fresh.close()


@pytest.mark.parametrize("name", [r.name for r in S.ROWS])
def test_row_matches_the_oracle_and_takes_its_branch(ctx, name):
    row = S.ROW[name]
    ran = run_row(ctx, row)
    want = ran["want"][ran["which"]]
    for exact in (False, True):
        got, plan = ran[exact]
        worst = float(np.max(np.abs(got - want)))
        print(name, "exact mode" if exact else "fast mode", plan, "worst |gpu - oracle|", worst)
        assert plan == S.words(row.plan(exact)), (name, exact, plan)
        assert plan[S.KERNEL] == S.EXACT if exact else plan[S.KERNEL] in (S.EXACT, S.FAST)
        assert got.shape == (row.pairs,) and worst <= S.BAR[plan[S.KERNEL]], (name, exact, plan, worst)
        for j in range(row.distinct):                       # pairs of the same images: the same bits, wherever they lie in the launch
            assert len(np.unique(got[ran["which"] == j])) == 1, (name, exact, j)
    assert np.max(np.abs(ran[False][0] - ran[True][0])) <= 1e-5, name
    # the branch the row is there for, in the mode it was worked out for
    plan = dict(zip(("kernel", "px", "aligned", "col_blocks", "block_cols", "band_rows", "bands", "why"), ran[row.exact][1]))
    plan["items_per_pair"] = plan["col_blocks"] * plan["bands"]
    for key, value in row.want.items():
        assert plan[key] == value, (name, key, plan)


def test_the_rows_cover_every_branch_of_the_plan(ctx):
    """A condition on the rows, not a measurement: what ke_last_ssim_plan reported over the whole table."""
    seen = [(row, exact, run_row(ctx, row)[exact][1]) for row in S.ROWS for exact in (False, True)]
    assert all(p[S.KERNEL] in (S.EXACT, S.FAST) for _, _, p in seen)
    combos = {(p[S.KERNEL], row.channels, p[S.PX], p[S.ALIGNED], p[S.COL_BLOCKS] > 1) for row, _, p in seen}
    every = {(k, ch, px, al, multi) for k in (S.EXACT, S.FAST) for ch in (1, 3, 4) for px in (4, 8) for al in (0, 1) for multi in (False, True)}
    assert len(every) == 48 and not every - combos, sorted(every - combos)
    for kernel in (S.EXACT, S.FAST):
        plans = [(row, p) for row, _, p in seen if p[S.KERNEL] == kernel]
        assert {S.TAKEN, S.WIDTH, S.BASE, S.BLOCKS} == {p[S.WHY] for _, p in plans}, kernel
        assert any(p[S.BANDS] == 1 for _, p in plans) and any(p[S.BANDS] >= 2 for _, p in plans), kernel
        assert any((row.h - 6) % p[S.BAND_ROWS] for row, p in plans if p[S.BANDS] >= 2), kernel            # a partial last band
        # several blocks and several bands at once, at either loader
        assert {p[S.ALIGNED] for _, p in plans if p[S.BANDS] >= 2 and p[S.COL_BLOCKS] >= 2} == {0, 1}, kernel
        assert any(row.base and p[S.WHY] == S.BASE for row, p in plans) and any(row.base and p[S.WHY] == S.WIDTH for row, p in plans), kernel
        assert any(row.pairs > 1 and p[S.COL_BLOCKS] * p[S.BANDS] == 3 for row, p in plans), kernel         # pairs share a workgroup
    fast = [(row, p) for row, _, p in seen if p[S.KERNEL] == S.FAST]
    heights = {p[S.BAND_ROWS] for _, p in fast}
    assert {14, 126} <= heights and any(14 < v < 126 for v in heights), heights
    assert all(v % 7 == 0 for v in heights)
    assert any((row.h - 6) % 7 for row, _ in fast)                                                          # a partial last group of seven rows
    assert any((row.h - 6) % 7 and p[S.BANDS] >= 2 for row, p in fast)
    assert all(p[S.BAND_ROWS] == 64 for _, _, p in seen if p[S.KERNEL] == S.EXACT)
    # the worst difference per kernel over the table
    for kernel, label in ((S.EXACT, "exact"), (S.FAST, "fast")):
        worst = max(float(np.max(np.abs(run_row(ctx, row)[exact][0] - run_row(ctx, row)["want"][run_row(ctx, row)["which"]])))
                    for row, exact, p in seen if p[S.KERNEL] == kernel)
        print(f"worst |gpu - oracle| of the {label} kernel over the table: {worst:.3e}")


@pytest.mark.parametrize("name", ["shared_exact_756x7", "shared_fast_756x12"])
def test_an_image_against_itself_scores_one(ctx, name):
    """Five pairs (a, a) of three waves each: 1.0 to the bit from the exact kernel, within 1e-7 from the fast one."""
    row = S.ROW[name]
    px = S.pixels(row)
    k = 2 * np.arange(row.pairs)
    for exact in (False, True):
        got, plan = score(ctx, row, px, k, k, exact)
        assert plan[S.COL_BLOCKS] * plan[S.BANDS] == 3 and got.shape == (5,)
        if plan[S.KERNEL] == S.EXACT:
            assert np.array_equal(got, np.ones(5)), (name, exact, got)
        else:
            assert np.max(np.abs(got - 1.0)) <= 1e-7, (name, exact, got)


@pytest.mark.parametrize("w,h", S.NAN_SHAPES)
def test_a_side_under_seven_scores_nan(ctx, w, h):
    rng = np.random.default_rng(w * 16 + h)
    for ch in (1, 3, 4):
        px = rng.integers(0, 256, (4, h, w, ch), dtype=np.uint8)
        for exact in (False, True):
            with time_limit():
                ctx.ssim_set_mode(exact)
                try:
                    got = ctx.ssim_pairs_uniform(px[..., 0].copy() if ch == 1 else px, 4, w, h, ch, [0, 1, 2], [1, 2, 3])
                    plan = ctx.last_ssim_plan()
                finally:
                    ctx.ssim_set_mode(False)
            assert got.shape == (3,) and np.isnan(got).all() and plan == (S.NAN,) + (-1,) * 7, (w, h, ch, exact, plan)
