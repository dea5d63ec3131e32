"""The launch plan of the SSIM kernels without a GPU: csrc/ke_ssim_plan.h compiled with the host C++ compiler
(tests/_ssim_plan_cpu.cpp) into a temporary directory, held against the rules written out a second time in
tests/_ssim_plan_cases.py (``plan``; its docstring states them, and nothing of it is read from the header).

The sweep: every width 7..3100 at heights 7, 8, 12, 13, 14, 20, 21, 69, 70, 71, 132, 133, 134 and 512, with 1, 2, 39, 2048, 3200,
8192 and 11700 pairs, the base address at every residue modulo 4, 1, 3 and 4 channels, in both modes.  What any plan must satisfy,
whatever the rules make of it, is asserted on the header's own words.  The same source has a ``main`` that walks the sweep (and the
sides under 7) with those conditions; it is built with AddressSanitizer and UBSan and run as a program of its own."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _ssim_plan_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "_ssim_plan_cpu.cpp")
WIDTHS = np.arange(7, 3101, dtype=np.int32)
HEIGHTS = (7, 8, 12, 13, 14, 20, 21, 69, 70, 71, 132, 133, 134, 512)
PAIRS = (1, 2, 39, 2048, 3200, 8192, 11700)
CHANNELS = (1, 3, 4)
FIELDS = ("kernel", "px", "aligned", "col_blocks", "block_cols", "band_rows", "bands", "items_per_pair", "n_items", "why")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ssim_plan_cpu") / "ssim_plan_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC, SOURCE, "-o", out])
    lib = C.CDLL(out)
    lib.sp_plan_many.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
    lib.sp_plan_many.restype = None
    return lib


def planned(cpu, widths, h, channels, pairs, base, exact) -> dict:
    """The header's plans of the widths as arrays, one per field."""
    widths = np.ascontiguousarray(widths, np.int32)
    out = np.empty((len(widths), len(FIELDS)), np.int64)
    cpu.sp_plan_many(widths.ctypes.data, len(widths), h, channels, pairs, base, int(exact), out.ctypes.data)
    return {name: out[:, k] for k, name in enumerate(FIELDS)}


def sweep():
    return [(h, ch, pairs, base, exact) for h in HEIGHTS for ch in CHANNELS for pairs in PAIRS for base in range(4) for exact in (False, True)]


def test_the_header_plans_every_shape_of_the_sweep_as_the_rules_do(cpu):
    for h, ch, pairs, base, exact in sweep():
        got, want = planned(cpu, WIDTHS, h, ch, pairs, base, exact), S.plan(WIDTHS, h, ch, pairs, base, exact)
        for name in FIELDS:
            bad = np.flatnonzero(got[name] != want[name])
            assert not len(bad), (name, int(WIDTHS[bad[0]]), h, ch, pairs, base, exact, int(got[name][bad[0]]), int(want[name][bad[0]]))


def test_what_any_plan_must_satisfy(cpu):
    w = WIDTHS.astype(np.int64)
    seen = set()
    for h, ch, pairs, base, exact in sweep():
        p = planned(cpu, WIDTHS, h, ch, pairs, base, exact)
        where = (h, ch, pairs, base, exact)
        fast = p["kernel"] == S.FAST
        assert np.all(fast | (p["kernel"] == S.EXACT)), where
        assert np.all((p["px"] == 4) | (p["px"] == 8)), where
        # blocks tile the interior columns exactly once, bands the interior rows
        assert np.all(((p["col_blocks"] - 1) * p["block_cols"] < w - 6) & (w - 6 <= p["col_blocks"] * p["block_cols"])), where
        assert np.all(((p["bands"] - 1) * p["band_rows"] < h - 6) & (h - 6 <= p["bands"] * p["band_rows"])), where
        assert np.all((p["aligned"] == 0) | (p["block_cols"] % 4 == 0) | (p["col_blocks"] == 1)), where
        assert np.all((p["aligned"] == 0) | ((w % 4 == 0) & (base == 0))), where
        assert np.all((p["aligned"] == 1) == (p["why"] == S.TAKEN)) and np.all((p["why"] >= S.TAKEN) & (p["why"] <= S.BLOCKS)), where
        assert np.all(p["block_cols"] <= 64 * p["px"] - 6), where
        assert np.all(~fast | ((p["band_rows"] % 7 == 0) & (p["band_rows"] >= 14) & (p["band_rows"] <= 126))), where
        assert np.all(fast | (p["band_rows"] == 64)), where
        assert np.all(((w - 6) * (h - 6) >= 4096) | ~fast), where
        assert not (exact and fast.any()), where
        assert np.all((p["items_per_pair"] == p["col_blocks"] * p["bands"]) & (p["n_items"] == pairs * p["items_per_pair"])), where
        seen.update(zip(p["kernel"].tolist(), p["px"].tolist(), p["aligned"].tolist(), (p["col_blocks"] > 1).tolist()))
        seen.update(("why", v) for v in np.unique(p["why"]).tolist())
        seen.update(("band_rows", v) for v in np.unique(p["band_rows"][fast]).tolist())
    # the sweep itself reaches every branch: both kernels x 4 or 8 pixels x either loader x one or several blocks, ...
    assert {k for k in seen if len(k) == 4} == {(k, px, al, m) for k in (S.EXACT, S.FAST) for px in (4, 8) for al in (0, 1) for m in (False, True)}
    assert {v for (k, *rest) in seen if k == "why" for v in rest} == {S.TAKEN, S.WIDTH, S.BASE, S.BLOCKS}
    heights = {v for (k, *rest) in seen if k == "band_rows" for v in rest}
    assert {14, 126} <= heights and len(heights) > 6


def test_a_side_under_seven_is_filled_with_nan(cpu):
    for small in range(1, 7):
        for other in (1, 6, 7, 64, 3100):
            for exact in (False, True):
                for w, h in ((small, other), (other, small)):
                    got = planned(cpu, [w], h, 3, 5, 0, exact)
                    assert got["kernel"][0] == S.NAN and all(got[name][0] == -1 for name in FIELDS[1:]), (w, h, exact)
                    assert S.plan(w, h, 3, 5, 0, exact)["kernel"] == S.NAN
    assert planned(cpu, [7], 7, 1, 1, 0, False)["kernel"][0] == S.EXACT


def test_the_widths_named_for_a_branch_take_it(cpu):
    """The smallest width of each layout, in exact mode at one row of windows."""
    want = {64: (4, 1, 1, 250, S.TAKEN), 63: (4, 0, 1, 250, S.WIDTH), 504: (4, 0, 2, 250, S.BLOCKS), 756: (4, 0, 3, 250, S.BLOCKS),
            760: (4, 1, 4, 248, S.TAKEN), 512: (8, 1, 1, 506, S.TAKEN), 509: (8, 0, 1, 506, S.WIDTH), 1012: (8, 1, 2, 504, S.TAKEN),
            1512: (8, 1, 3, 504, S.TAKEN), 1016: (8, 0, 2, 506, S.BLOCKS), 1010: (8, 0, 2, 506, S.WIDTH), 1008: (8, 1, 2, 504, S.TAKEN),
            1516: (8, 1, 3, 504, S.TAKEN), 1520: (8, 0, 3, 506, S.BLOCKS)}
    p = planned(cpu, list(want), 7, 1, 1, 0, True)
    for k, w in enumerate(want):
        assert tuple(int(p[name][k]) for name in ("px", "aligned", "col_blocks", "block_cols", "why")) == want[w], w
    # the band height follows the pairs in the launch: 64 x 132 luma
    for pairs, band_rows, bands in ((1, 14, 9), (2048, 28, 5), (3200, 42, 3), (8192, 126, 1)):
        p = planned(cpu, [64], 132, 1, pairs, 0, False)
        assert (p["kernel"][0], p["band_rows"][0], p["bands"][0]) == (S.FAST, band_rows, bands), pairs


def test_the_rows_of_the_gpu_table_are_planned_as_they_say(cpu):
    for row in S.ROWS:
        got = planned(cpu, [row.w], row.h, row.channels, row.pairs, row.base, row.exact)
        assert {name: int(got[name][0]) for name in FIELDS} == row.plan(row.exact), row.name
        for name, value in row.want.items():
            assert got[name][0] == value, (row.name, name, int(got[name][0]))


def test_sanitised_program(tmp_path):
    exe = str(tmp_path / "ssim_plan_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-DSSIM_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", CSRC, SOURCE, "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    plans = 3100 * len(HEIGHTS) * len(CHANNELS) * len(PAIRS) * 4 * 2
    assert done.stdout.strip() == f"ok {plans}" and "runtime error" not in done.stderr
