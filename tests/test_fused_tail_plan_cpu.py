"""The plan of the single-pass kernels' matrix-core tail (ke_plan_fused_tail, csrc/ke_resample_plan.h) without a GPU: the
header compiled with the host C++ compiler (tests/_fused_tail_plan_cpu.cpp, linked with csrc/ke_coeffs.cpp for the real tables).

tests/test_resample_plan_cpu.py holds ke_plan_fused to its recording; this file holds what the tail adds to that plan to
what the kernel needs, stated from the kernel's reads and not from the header's arithmetic:
  * a step reads rows [base + 64 s, base + 64 s + 64) of every column, s < ks, so a column is at least max(base) + 64 ks
    bytes long (4 * kdq * 64 for the 8-output axis, whose window starts at row 0), and no shorter than before;
  * the reads are 16 bytes wide and the 16 columns of an operand should fall into distinct bank groups: the pitch is an
    odd number of 16-byte units;
  * the tables are built for whole groups of steps (3; 2 per wave on the dHash axis) and for no more than a group beyond
    what the axis needs;
  * the areas behind the columns move with them and the launch's LDS is their sum;
  * the longer columns never cost the second workgroup of a CU (80 KB each) nor pass 150 KB: such shapes keep the
    dot-product tail with ke_plan_fused's plan untouched, and so does every shape under KE_VTILE_VALU."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")

F = {name: k for k, name in enumerate(
    ["row", "why", "wide", "dh", "lt_half", "p_hp", "p_hpd", "p_x_off", "p_lds", "p_raise", "nat_ks", "base_max", "nat_ksd", "on_mx", "hp", "hpd",
     "x_off", "lds", "raise", "ks", "kdq", "valu_on_mx", "valu_same", "table_ks"])}


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("fused_tail_plan_cpu") / "fused_tail_plan_cpu.so")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC,
                           os.path.join(ROOT, "tests", "_fused_tail_plan_cpu.cpp"), os.path.join(CSRC, "ke_coeffs.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.ft_case.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    assert lib.ft_fields() == len(F)
    return lib


def plans(lib, w, h, want_d):
    out = np.zeros((4, len(F)), np.int64)
    n = lib.ft_case(w, h, int(want_d), out.ctypes.data)
    return [{name: int(out[k, i]) for name, i in F.items()} for k in range(n)]


def lds_of(wide, dh, lt_half, hp, hpd):
    """The areas of a single-pass workgroup in order: two tile buffers, 32 columns, 9 dHash columns, the exchange area."""
    lds = 2 * lt_half + 32 * hp
    if not wide:
        lds = max(lds, 4096)
    if dh:
        lds += 9 * hpd
    x_off = 0
    if wide or dh:
        lds = (lds + 15) // 16 * 16
        x_off = lds
        lds += (12 * 1024 + (14 * 1024 if dh else 0)) if wide else 4096
    return lds, x_off


def check(p, where):
    assert p["valu_on_mx"] == 0 and p["valu_same"] == 1, where
    assert lds_of(p["wide"], p["dh"], p["lt_half"], p["p_hp"], p["p_hpd"]) == (p["p_lds"], p["p_x_off"]), where
    # the tables the tail is handed
    assert p["table_ks"] % 3 == 0 and 0 <= p["table_ks"] - p["nat_ks"] < 3, where
    need_hp = max(p["p_hp"], p["base_max"] + 64 * p["table_ks"])
    kdq = -(-p["nat_ksd"] // 4)
    kdq += kdq % 2
    need_hpd = max(p["p_hpd"], 64 * 4 * kdq) if p["dh"] else p["p_hpd"]
    if not p["on_mx"]:
        # only for LDS: the shortest columns that serve would cost the second workgroup, or pass the kernel's limit
        assert (p["hp"], p["hpd"], p["x_off"], p["lds"], p["raise"]) == (p["p_hp"], p["p_hpd"], p["p_x_off"], p["p_lds"], p["p_raise"]), where
        odd16 = lambda b: ((b + 15) // 16 | 1) * 16
        least, _ = lds_of(p["wide"], p["dh"], p["lt_half"], odd16(need_hp), odd16(need_hpd) if p["dh"] else need_hpd)
        assert least > 150 * 1024 or (p["p_lds"] <= 80 * 1024 < least), where
        return
    assert p["ks"] == p["table_ks"], where
    assert p["hp"] % 32 == 16 and need_hp <= p["hp"] < need_hp + 32, where
    if p["dh"]:
        assert p["kdq"] == kdq, where
        assert p["hpd"] % 32 == 16 and need_hpd <= p["hpd"] < need_hpd + 32, where
    else:
        assert p["kdq"] == 0 and p["hpd"] == p["p_hpd"], where
    assert (p["lds"], p["x_off"]) == lds_of(p["wide"], p["dh"], p["lt_half"], p["hp"], p["hpd"]), where
    assert p["lds"] <= 150 * 1024 and (p["p_lds"] > 80 * 1024 or p["lds"] <= 80 * 1024), where
    assert p["raise"] == (p["lds"] > 64 * 1024), where


def test_the_benchmark_shape(cpu):
    """512 x 512, both hashes: 5 steps per block (windows of 16 * 16 + 96 rows from rows 0 and 192), built for 6; the columns
    must reach 192 + 6 * 64 = 576 bytes, 592 as an odd number of 16-byte units; 8 dHash steps, 2 per wave, need no more than the
    512 rows; two workgroups still share a CU."""
    (p,) = plans(cpu, 512, 512, True)
    assert (p["why"], p["dh"], p["wide"]) == (0, 1, 0)
    assert (p["nat_ks"], p["base_max"], p["nat_ksd"]) == (5, 192, 8) and p["p_hp"] < 576
    assert (p["on_mx"], p["ks"], p["kdq"], p["hp"]) == (1, 6, 2, 592)
    assert p["lds"] <= 80 * 1024 and not p["raise"]
    check(p, "512x512")


def test_every_shape_of_the_gpu_test(cpu):
    """tests/test_gpu_fused_tail.py: each of its RGB shapes that a single-pass kernel takes runs the matrix-core tail.  256 x 3000 is not
    among them (its columns fit LDS only per band); 1843 and 1274 rows are the most a 256-pixel row runs in one pass with this tail,
    for one hash and for both: 18 steps per block, and 12 with 6 dHash steps per wave."""
    for w, h, taken in [(256, 256, True), (512, 512, True), (68, 40, True), (700, 95, True), (70, 33, True), (128, 7, False), (128, 31, True),
                        (256, 65, True), (256, 127, True), (256, 3000, False), (256, 1843, True), (256, 1274, True), (1024, 64, True), (2048, 48, True),
                        (1100, 40, True)]:
        for want_d in (False, True):
            got = [p for p in plans(cpu, w, h, want_d) if p["why"] == 0]
            # both hashes of a 256 x 1843 image fit one workgroup no more: that call runs per band
            assert bool(got) == (taken and not (want_d and h == 1843)), (w, h, want_d)
            for p in got[:1]:                    # the row that runs
                check(p, (w, h, want_d))
                # 2048-pixel rows, pHash alone: two 16-row tile buffers and the exchange area leave 80 KB no room for
                # longer columns, and the shape keeps the dot-product tail (check() holds it to that reason)
                assert p["on_mx"] == (0 if (w, want_d) == (2048, False) else 1), (w, h, want_d)
                if h == 1843 and not want_d:
                    assert (p["dh"], p["ks"]) == (0, 18)
                if h == 1274 and want_d:
                    assert (p["dh"], p["ks"], p["kdq"]) == (1, 12, 6)


def test_sweep(cpu):
    heights = [16, 17, 31, 33, 40, 63, 64, 65, 95, 127, 128, 256, 333, 512, 700, 1000, 1200, 1536, 2048, 2500, 3000, 4096]
    widths = list(range(65, 2100, 37)) + [68, 256, 384, 512, 516, 704, 708, 768, 1024, 1536, 2048, 2560, 2816]
    seen = {"mx": 0, "valu_80k": 0, "dh": 0, "wide": 0, "one_per_cu": 0}
    for h in heights:
        for w in widths:
            for want_d in (False, True):
                for p in plans(cpu, w, h, want_d):
                    if p["why"]:
                        continue
                    check(p, (w, h, want_d, p["row"]))
                    seen["mx"] += p["on_mx"]
                    seen["valu_80k"] += not p["on_mx"]
                    seen["dh"] += p["on_mx"] and p["dh"]
                    seen["wide"] += p["on_mx"] and p["wide"]
                    seen["one_per_cu"] += p["on_mx"] and p["p_lds"] > 80 * 1024
    assert all(seen.values()), seen              # every branch of the plan was met
