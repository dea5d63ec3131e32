"""How the resample kernels are launched, without a GPU: csrc/ke_resample_plan.h compiled with the host C++ compiler
(tests/_resample_plan_cpu.cpp, linked with csrc/ke_coeffs.cpp for the real coefficient, chunk and operand tables) into a
temporary directory.

Every field of every plan is held to tests/golden/resample_plans.json, recorded from the arithmetic that stood between the
launches of csrc/ke_hash.hip before the header existed (tests/golden/README), never from the header: the sweep of SWEEP below,
and the shapes of the GPU tests that steer the plans one by one.  There is no tolerance."""
from __future__ import annotations

import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "resample_plans.json")

LANCZOS, BILINEAR, BICUBIC = 0, 1, 2
SWEEP = {
    "widths": [1, 8200],
    "heights": [1, 3, 16, 17, 64, 600, 4001, 5000],
    "targets": [[32, 32], [9, 8], [128, 128], [300, 129]],
    "channels": [1, 3, 4],
    "ns": [1, 3, 200, 5000],
}
# Inside a record the switches and the CU count take every value they have: KE_VTILE_VALU unset / set, KE_FUSED_MIN_IMAGES
# unset / 1 / 1000, 8 and 256 CUs, one hash or both, one workgroup per image or per band.

# tests/test_gpu_resample.py ROWS: name, w, h, n, targets, channels (every row runs the three filters)
RESAMPLE_ROWS = [
    ("up_both", 64, 64, 3, [(100, 90)], (1, 3, 4)), ("up_down", 100, 64, 3, [(64, 100)], (1, 3, 4)),
    ("identity_axis", 300, 200, 3, [(300, 77), (77, 200)], (1, 3, 4)), ("ndwc16", 640, 96, 3, [(128, 33)], (1, 3, 4)),
    ("funnel_valu", 641, 97, 3, [(129, 129)], (1, 3, 4)), ("launch_of_one", 600, 300, 3, [(257, 128), (300, 129)], (1, 3, 4)),
    ("ndw32", 2340, 24, 3, [(130, 12), (128, 12)], (1,)), ("cpo2_funnel", 1170, 24, 3, [(64, 24)], (3,)),
    ("ndwc24", 3000, 40, 3, [(300, 40)], (1, 3, 4)), ("cpo16_l", 4096, 40, 3, [(16, 17)], (1, 3, 4)),
    ("cpo16_c", 4096, 40, 3, [(16, 16)], (1, 3, 4)), ("cpo32", 8192, 8, 3, [(12, 8)], (1,)),
    ("cpo32_funnel", 8190, 8, 3, [(13, 8)], (3,)), ("window_too_long", 8192, 8, 3, [(12, 8)], (1,)),
    ("row_too_long", 8196, 8, 3, [(64, 8)], (1,)), ("lds_too_large", 16, 600, 3, [(64, 64)], (1,)),
    ("lds_fits", 16, 200, 3, [(64, 64)], (1,)), ("mfma_63_steps", 40, 4000, 3, [(20, 16)], (1,)),
    ("vertical_first", 40, 4001, 3, [(20, 16)], (1,)), ("px_1x3", 1, 3, 3, [(4, 4)], (1,)), ("px_3x1", 3, 1, 3, [(4, 4)], (1,)),
    ("px_1x1", 1, 1, 3, [(4, 4)], (1,)), ("smallest_banded", 2, 2, 3, [(5, 5)], (1, 3, 4)), ("n3", 64, 200, 3, [(48, 50)], (1,)),
    ("n1500", 64, 200, 1500, [(48, 50)], (1,)), ("bands4", 64, 2000, 3, [(48, 127)], (1,)), ("bands32", 200, 5000, 3, [(100, 300)], (1,)),
    ("tile_edges", 96, 80, 3, [(ow, oh) for ow in (15, 16, 17) for oh in (15, 16, 17, 31, 32, 33)], (1, 3, 4)),
]
# tests/test_gpu_parity.py: test_phash_strip_kernel_for_rows_wider_than_2048 (n = 2, RGB) and test_banded_path_matches_oracle
STRIP_SHAPES = [(2816, 64), (3000, 33), (3072, 300), (3264, 17), (4000, 3000), (4032, 64), (4096, 500), (4608, 80), (5184, 48), (5296, 16),
                (2560, 100), (5400, 16)]
BANDED_SHAPES = [(1024, 768, 3, 6), (640, 480, 3, 8), (1000, 667, 3, 5), (333, 517, 3, 5), (2048, 1536, 3, 2), (4096, 4096, 3, 1), (768, 3072, 3, 2),
                 (100, 60, 3, 9), (37, 1000, 3, 4), (16, 16, 3, 7), (5, 4, 3, 3), (513, 512, 3, 4), (800, 600, 1, 4), (801, 603, 1, 3), (640, 360, 4, 4),
                 (1920, 1080, 3, 2), (3072, 256, 3, 2), (256, 4096, 3, 2), (8, 2048, 3, 2)]


def extra_cases():
    """(w, h, channels, n, misaligned, base on a dword, stride a multiple of 4, offset array, ow, oh, filter) one by one."""
    out = []
    for _name, w, h, n, targets, channels in RESAMPLE_ROWS:
        out += [(w, h, c, n, 0, 1, 1, 0, ow, oh, f) for c in channels for (ow, oh) in targets for f in (LANCZOS, BILINEAR, BICUBIC)]
    out += [(w, h, 3, 2, 0, 1, 1, 0, ow, oh, LANCZOS) for (w, h) in STRIP_SHAPES for (ow, oh) in ((32, 32), (9, 8))]
    out += [(w, h, c, n, 0, 1, 1, 0, ow, oh, LANCZOS) for (w, h, c, n) in BANDED_SHAPES for (ow, oh) in ((32, 32), (9, 8))]
    for (ow, oh) in ((32, 32), (9, 8)):
        out += [(4000, 3000, 3, 200, 1, 1, 1, 1, ow, oh, LANCZOS),       # a ragged group with an image off a dword boundary
                (4000, 3000, 3, 200, 0, 0, 1, 0, ow, oh, LANCZOS),       # the base pointer off by 2
                (4000, 3000, 3, 200, 0, 1, 0, 0, ow, oh, LANCZOS),       # a stride that is no multiple of 4 ...
                (4000, 3000, 3, 200, 0, 1, 0, 1, ow, oh, LANCZOS),       # ... which an offset array makes irrelevant
                (16384, 50000, 3, 1, 0, 1, 1, 0, ow, oh, LANCZOS),       # 2 GiB and more
                (4000, 3000, 3, 3_000_000_000, 0, 1, 1, 0, ow, oh, LANCZOS),   # more workgroups than a launch takes
                (640, 480, 3, 3_000_000_000, 0, 1, 1, 0, ow, oh, LANCZOS),
                (640, 480, 3, 200, 1, 1, 1, 1, ow, oh, LANCZOS)]
    out += [(700, 65536, 1, 2, 0, 1, 1, 0, 64, 129, BILINEAR),           # one column of the VALU vertical pass over 64 KiB
            (2816, 2000, 3, 600, 0, 1, 1, 0, 32, 32, LANCZOS),           # a single-pass kernel over 150 KB of LDS
            (64, 64, 1, 3_000_000_000, 0, 1, 1, 0, 64, 64, BILINEAR),
            (64, 64, 1, 2_000_000_000, 0, 1, 1, 0, 64, 64, BILINEAR)]    # one launch of ke_hband, too many waves for ke_vtile_mx
    return out


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def load(path):
    lib = C.CDLL(path)
    lib.rp_case.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.rp_case.restype = C.c_int64
    lib.rp_sweep.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.rp_sweep.restype = C.c_int64
    lib.rp_result.argtypes = [C.c_void_p]
    lib.rp_seen.argtypes = [C.c_void_p]
    return lib


def key_text(key):
    """A key as the fixture holds it: the values with commas between, -1 (no answer) as nothing."""
    return ",".join("" if v == -1 else str(int(v)) for v in key)


KEY_PARTS = [(0, 9), (9, 25), (25, 57), (57, 61)]       # banded path and its vertical pass; strips and bands; single-pass rows; the rest


def split_key(text):
    fields = text.split(",")
    assert len(fields) == KEY_PARTS[-1][1]
    return [",".join(fields[a:b]) for a, b in KEY_PARTS]


def fixture_keys(golden):
    """The fixture holds a key as four indices into "parts"."""
    return [",".join(golden["parts"][p] for p in key) for key in golden["keys"]]


def run_case(lib, case):
    """(the whole record, its key, its digest)"""
    v = np.asarray(case, np.int64)
    out, key, digest = np.zeros(4096, np.int64), np.zeros(lib.rp_key_ints(), np.int32), C.c_uint64(0)
    n = lib.rp_case(v.ctypes.data, out.ctypes.data, out.size, key.ctypes.data, C.byref(digest))
    assert n <= out.size
    return out[:n].tolist(), key_text(key), f"{digest.value:016x}"


def run_sweep(lib, sweep=SWEEP):
    """[(sequence name, digest, [(first width, last width, key), ...])] in the order heights x targets x channels x ns x (other, aligned)"""
    h, t = np.asarray(sweep["heights"], np.int32), np.asarray(sweep["targets"], np.int32).reshape(-1)
    c, n = np.asarray(sweep["channels"], np.int32), np.asarray(sweep["ns"], np.int64)
    size = lib.rp_sweep(sweep["widths"][0], sweep["widths"][1], h.ctypes.data, h.size, t.ctypes.data, t.size // 2, c.ctypes.data, c.size, n.ctypes.data, n.size)
    flat = np.zeros(size, np.int64)
    lib.rp_result(flat.ctypes.data)
    k, at, out = lib.rp_key_ints(), 0, []
    while at < size:
        hh, ow, oh, cc, nn, aligned, digest, runs = flat[at:at + 8].tolist()
        body = flat[at + 8:at + 8 + runs * (k + 2)].reshape(runs, k + 2)
        out.append((f"h{hh} t{ow}x{oh} c{cc} n{nn} {'aligned' if aligned else 'other'}", f"{digest & (2**64 - 1):016x}",
                    [(int(r[0]), int(r[1]), key_text(r[2:])) for r in body]))
        at += 8 + runs * (k + 2)
    return out


def spelled_out(cases):
    """The extra cases whose whole record the fixture spells out: the first of each source shape."""
    first = {}
    for k, case in enumerate(cases):
        first.setdefault(case[:2], k)
    return sorted(first.values())


def seen(lib):
    out = np.zeros((6, 32), np.int64)
    lib.rp_seen(out.ctypes.data)
    return out


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resample_plan_cpu") / "resample_plan_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC,
                           os.path.join(ROOT, "tests", "_resample_plan_cpu.cpp"), os.path.join(CSRC, "ke_coeffs.cpp"), "-o", out])
    lib = load(out)
    lib.rp_why_name.argtypes = [C.c_int]
    lib.rp_why_name.restype = C.c_char_p
    lib.rp_entry_name.argtypes = [C.c_int]
    lib.rp_entry_name.restype = C.c_char_p
    lib.rp_entry_calls.argtypes = [C.c_int]
    lib.rp_entry_calls.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


# what each path can answer: 0 = it takes the shape
PATHS = ["hband", "vtile", "strips", "sp_bands", "fused", "generic"]
ANSWERS = {
    "hband": {"OK", "ONE_LAUNCH", "HB_VERTICAL_FIRST", "HB_SHAPE", "HB_WINDOW", "HB_ROW", "HB_LDS"},
    "vtile": {"OK", "ONE_LAUNCH", "VT_LDS"},
    "strips": {"OK", "ONE_LAUNCH", "ST_TARGET", "ST_SHAPE", "ST_ADDRESS", "ST_STEPS", "ST_LAST_STRIP", "ST_SWITCH", "ST_FILL"},
    "sp_bands": {"OK", "SPB_SHAPE"},
    "fused": {"OK", "ONE_LAUNCH", "FU_WIDTH", "FU_LDS", "FU_BANDS_FIT"},
    "generic": {"OK"},
}
# Three declines guard against a table that ke_coeffs.cpp does not build for the step counts the plan itself asked for: they
# stand in the header as they stood in the launchers, and no real table reaches them (so the recording found, too).
UNREACHED = {"ST_TABLE", "FU_TABLE", "FU_DH_TABLE"}


def test_every_plan_is_the_recorded_one(cpu, golden):
    assert {k: golden[k] for k in SWEEP} == SWEEP
    got = run_sweep(cpu)
    assert len(got) == len(golden["sequences"]) == len(SWEEP["heights"]) * len(SWEEP["targets"]) * len(SWEEP["channels"]) * len(SWEEP["ns"]) * 2 == 768
    widths = range(SWEEP["widths"][0], SWEEP["widths"][1] + 1)
    keys = fixture_keys(golden)
    cases = 0
    for (name, digest, runs), (at, want_digest) in zip(got, golden["sequences"]):
        want = [(first, last, keys[k]) for first, last, k in golden["runlists"][at]]
        assert runs == want, name                    # the decisions, width by width
        assert digest == want_digest, name           # every field of every record of the sequence
        mine = [w for w in widths if (w % 4 == 0) == name.endswith("aligned")]
        at = {w: k for k, w in enumerate(mine)}          # the runs tile the sequence's widths, in order, with no gap
        assert runs[0][0] == mine[0] and runs[-1][1] == mine[-1] and all(at[b[0]] == at[a[1]] + 1 for a, b in zip(runs, runs[1:])), name
        cases += len(mine)
    assert cases == 8200 * 384
    extras = extra_cases()
    assert len(golden["extra"]) == len(extras) and sorted(map(int, golden["extra_records"])) == spelled_out(extras)
    for k, (case, (key, want_digest)) in enumerate(zip(extras, golden["extra"])):
        record, got_key, digest = run_case(cpu, case)
        assert (got_key, digest) == (keys[key], want_digest), case
        if str(k) in golden["extra_records"]:
            assert record == golden["extra_records"][str(k)], case
    # every answer of every path occurs, and so does every entry point of the header
    names = [cpu.rp_why_name(k).decode() for k in range(cpu.rp_why_count())]
    assert set().union(*ANSWERS.values()) | UNREACHED == set(names)
    counts = seen(cpu)
    for p, path in enumerate(PATHS):
        assert {names[k] for k in range(len(names)) if counts[p, k]} == ANSWERS[path], path
    assert golden["seen"] == {path: {names[k]: int(counts[p, k]) for k in range(len(names)) if counts[p, k]} for p, path in enumerate(PATHS)}
    entries = {cpu.rp_entry_name(k).decode(): cpu.rp_entry_calls(k) for k in range(cpu.rp_entry_count())}
    assert len(entries) == 17 and all(entries.values()), entries
