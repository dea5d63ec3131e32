"""The visibility condition on the inputs of tests/test_gpu_ssim_plan.py, without a GPU: a score is a mean over thousands of
windows, so a window dropped, doubled or read from the neighbouring lane or row at a seam of the launch plan shows only if the
SSIM map steps there.  For every row of the table, in both modes, the map of its inputs is computed in plain float64 NumPy
(``ssim_map`` of tests/_ssim_plan_cases.py: the reference, not the kernel), and each of these must move the mean by at least four
times the bar the row's kernel is held to:

- a map column on either side of a block seam set to zero, or replaced by either of its neighbours;
- the same for the map rows on either side of a band seam;
- for the family "lanes", the same for the first and last map column and row (the picture's edges).

A row that fails needs a smaller height, not a smaller factor."""
from __future__ import annotations

import numpy as np
import pytest

import _ssim_plan_cases as S

FACTOR = 4.0


def maps(row: S.Row) -> list:
    px = S.luma(S.pixels(row))
    return [S.ssim_map(px[2 * k], px[2 * k + 1]) for k in range(row.distinct)]


def lines(row: S.Row, p: dict, size: int, axis: int) -> list:
    """The map columns (axis 1) or rows (axis 0) under test."""
    if row.family == "lanes":
        return [0, size - 1]
    step, count = (p["block_cols"], p["col_blocks"]) if axis == 1 else (p["band_rows"], p["bands"])
    return [k * step + d for k in range(1, count) for d in (-1, 0)]


def weakest(m: np.ndarray, line: int, axis: int) -> float:
    """The smallest change of the mean from zeroing the line or replacing it by a neighbour."""
    m = m if axis == 0 else m.T
    moves = [abs(m[line].sum())] + [abs((m[line] - m[nb]).sum()) for nb in (line - 1, line + 1) if 0 <= nb < len(m)]
    return min(moves) / m.size


@pytest.mark.parametrize("name", [r.name for r in S.ROWS])
def test_a_wrong_window_at_a_seam_moves_the_score(name):
    row = S.ROW[name]
    ms = maps(row)
    worst = None
    for mode in (False, True):
        p = row.plan(mode)
        need = FACTOR * S.BAR[p["kernel"]]
        for m in ms:
            assert m.shape == (row.h - 6, row.w - 6)
            for axis in (0, 1):
                for line in lines(row, p, m.shape[axis], axis):
                    ratio = weakest(m, line, axis) / S.BAR[p["kernel"]]
                    worst = ratio if worst is None else min(worst, ratio)
                    assert weakest(m, line, axis) >= need, (name, "exact" if mode else "fast", "row" if axis == 0 else "column", line, ratio)
    print(name, "smallest move / bar:", worst)


def test_the_map_is_skimage_s():
    """The float64 restatement against the definition on one window, and a score of 1 for equal images."""
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (7, 7)), rng.integers(0, 256, (7, 7))
    x, y = a / 255.0, b / 255.0
    ux, uy = x.mean(), y.mean()
    vx, vy, vxy = x.var(ddof=1), y.var(ddof=1), ((x - ux) * (y - uy)).sum() / 48.0
    want = (2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    assert abs(S.ssim_map(a, b)[0, 0] - want) < 1e-12
    big = rng.integers(0, 256, (20, 33))
    assert S.ssim_map(big, big).shape == (14, 27) and np.allclose(S.ssim_map(big, big), 1.0, atol=1e-12)


def test_the_inputs_step_at_every_seam():
    """Strength 0 leaves b equal to a, and only that; the strength changes at pixel column seam + 3 and pixel row seam + 3 and nowhere else."""
    for row in S.ROWS:
        px, st = S.pixels(row), S.strength(row)
        assert px.shape[:3] == (2 * row.distinct, row.h, row.w) and px.dtype == np.uint8 and st.shape == (row.h, row.w)
        same = (px[0::2] == px[1::2]) if row.channels == 1 else (px[0::2] == px[1::2]).all(axis=-1)
        assert same[:, st == 0].all() and not same[:, st > 0].all() and set(np.unique(st)) <= {0, 1, 2}
        if row.family == "seams":
            cols, rows = S.seams(row)
            if cols or rows:
                assert (np.flatnonzero(np.diff(st[0])) + 1).tolist() == [c + 3 for c in cols], row.name      # (no seam above row 0 ...
                assert (np.flatnonzero(np.diff(st[:, 0])) + 1).tolist() == [r + 3 for r in rows], row.name   # ... or left of column 0)
