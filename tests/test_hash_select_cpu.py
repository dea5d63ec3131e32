"""Which single-pass hash kernel a shape gets, and how a ragged batch is cut into shape groups, without a GPU:
ke_hash_select.h and ke_group_plan.h compiled with the host C++ compiler (tests/_hash_select_cpu.cpp) into a temporary directory.

The candidate lists are held to tests/golden/hash_single_pass_candidates.json, recorded from the nested switches the table
replaced (tests/golden/README): every width 1..3000 x channels x one or both hashes x band plan or none x six heights, and
the rejections one by one.  The one licence: a row already tried in the same call is not tried a second time.  The group
planner is held to the two loops it replaced, restated literally below."""
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "hash_single_pass_candidates.json")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hash_select_cpu") / "hash_select_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC,
                           os.path.join(ROOT, "tests", "_hash_select_cpu.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.hsel_row.argtypes = [C.c_int, C.c_void_p]
    lib.hsel_candidates.argtypes = [C.c_int] * 6 + [C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    lib.hsel_sweep.argtypes = [C.c_int] * 6 + [C.c_void_p]
    lib.hsel_plan.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hsel_plan.restype = C.c_int64
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def _row_names(lib):
    names = []
    for r in range(lib.hsel_row_count()):
        v = np.zeros(9, np.int32)
        lib.hsel_row(r, v.ctypes.data)
        names.append(",".join(["mx" if v[0] == 0 else "wide"] + [str(int(x)) for x in v[1:7]]))
    return names


def _without_repeats(rows):
    return list(dict.fromkeys(rows))


def test_the_candidate_order_is_the_recorded_one(cpu, golden):
    names = _row_names(cpu)
    assert len(set(names)) == len(names) == 70
    w0, w1 = golden["widths"]
    seen, cases, repeats = set(), 0, 0
    for key, runs in golden["sweep"].items():
        c, d, p, h, which = key.split()
        c, d, p, h = int(c[1:]), int(d[1:]), int(p[1:]), int(h[1:])
        got = np.zeros((w1 - w0 + 1, 5), np.int32)
        cpu.hsel_sweep(c, d, p, h, w0, w1, got.ctypes.data)
        widths = [w for w in range(w0, w1 + 1) if (w % 4 == 0) == (which == "aligned")]
        at = 0
        for first, last, rows in runs:                            # the runs tile the sequence, in order, with no gap
            assert widths[at] == first, (key, first)
            want = _without_repeats([golden["rows"][r] for r in rows])
            repeats += len(rows) != len(want)
            while at < len(widths) and widths[at] <= last:
                n, *idx = got[widths[at] - w0].tolist()
                assert [names[r] for r in idx[:n]] == want, (key, widths[at])
                assert idx[n:] == [-1] * (4 - n)
                seen.update(idx[:n])
                cases += 1
                at += 1
        assert at == len(widths), key
    assert cases == 3 * 2 * 2 * len(golden["heights"]) * (w1 - w0 + 1) == 216000
    # the repeat rule is used where the issue says the old code tried one kernel twice, and nowhere else
    assert repeats > 0 and all(len(rows) == len(set(rows)) or (key.startswith("c3 d1 p1") and 708 <= first and last <= 768)
                               for key, runs in golden["sweep"].items() for first, last, rows in runs)
    # every row of the table is some shape's candidate, and the recorded rows are the table's: none unreachable, none missing
    assert seen == set(range(len(names)))
    assert sorted(golden["rows"]) == sorted(names)


def test_each_rejection_is_the_recorded_one(cpu, golden):
    names = _row_names(cpu)
    assert {e["name"] for e in golden["extra"]} == {"misaligned", "base_off_2", "stride_not_4", "stride_not_4_offsets", "tall", "2g", "below_2g"}
    for e in golden["extra"]:
        out = np.zeros(4, np.int32)
        stride = e["w"] * e["h"] * e["channels"] + e["stride_mod4"]
        n = cpu.hsel_candidates(e["w"], e["h"], e["channels"], e["misaligned"], e["base_mod4"], e["offsets"], stride, e["want_d"], e["plan"], out.ctypes.data)
        assert [names[r] for r in out[:n]] == _without_repeats([golden["rows"][r] for r in e["candidates"]]), e["name"]
        assert (n == 0) == (e["name"] not in ("stride_not_4_offsets", "below_2g")), e["name"]


def test_the_rows_say_what_they_take(cpu):
    """A row's own fields against the shapes it is listed for: channels, aligned or not, one hash or both, the width range."""
    seen = set()
    for c in (1, 3, 4):
        for d in (0, 1):
            got = np.zeros((3000, 5), np.int32)
            cpu.hsel_sweep(c, d, 1, 100, 1, 3000, got.ctypes.data)
            for w in range(1, 3001):
                n, *idx = got[w - 1].tolist()
                for k, r in enumerate(idx[:n]):
                    v = np.zeros(9, np.int32)
                    cpu.hsel_row(r, v.ctypes.data)
                    assert v[5] == c and bool(v[6]) == (w % 4 != 0) and v[7] <= w <= v[8], (r, w)
                    assert not v[3] or d, (r, w)                  # a both-hashes row only when both are wanted ...
                    assert not v[3] or k == 0, (r, w)             # ... and then first
                    seen.add(r)
    assert len(seen) == 70


# ---- the group planner against the two loops it replaced ------------------------------------------------------------
def _groups_as_hash_images_wrote_them(off, w, h, channels, take, base):
    """hash_images_impl's device-resident branch: a map keyed (w, h), members in input order, then the metadata loop."""
    groups = {}
    for i in range(len(w)):
        if take[i]:
            groups.setdefault((int(w[i]), int(h[i])), []).append(i)
    meta, out = [], []
    for key in sorted(groups):
        idx = groups[key]
        out.append((key[0], key[1], channels, len(meta), len(idx), int(any((base + int(off[i])) % 4 != 0 for i in idx))))
        meta += [int(off[i]) for i in idx] + idx
    return out, meta


def _groups_as_stage_submit_wrote_them(off, w, h, c, take, base):
    """ke_stage_submit_hash: a map keyed (w, h, c)."""
    groups = {}
    for i in range(len(w)):
        if take[i]:
            groups.setdefault((int(w[i]), int(h[i]), int(c[i])), []).append(i)
    meta, out = [], []
    for key in sorted(groups):
        idx = groups[key]
        out.append(key + (len(meta), len(idx), int(any((base + int(off[i])) % 4 != 0 for i in idx))))
        meta += [int(off[i]) for i in idx] + idx
    return out, meta


def _plan(lib, off, w, h, c, c_all, take, base):
    n = len(w)
    off, w, h = np.asarray(off, np.uint64), np.asarray(w, np.int32), np.asarray(h, np.int32)
    c = None if c is None else np.asarray(c, np.int32)
    take = np.asarray(take, np.uint8)
    meta = np.full(2 * n + 1, 0xABCD, np.uint64)
    groups = np.zeros((n + 1, 6), np.int64)
    words = C.c_uint64(0)
    ng = lib.hsel_plan(off.ctypes.data, w.ctypes.data, h.ctypes.data, None if c is None else c.ctypes.data, c_all, take.ctypes.data, n, base,
                       meta.ctypes.data, groups.ctypes.data, C.byref(words))
    assert meta[words.value:].tolist() == [0xABCD] * (2 * n + 1 - words.value)          # nothing written past what it reports
    return [tuple(g) for g in groups[:ng].tolist()], meta[:words.value].tolist()


def _hold(lib, off, w, h, c, take, base):
    """Both forms: one channel count for the call (each of 1, 3, 4), and channels per image."""
    for c_all in (1, 3, 4):
        assert _plan(lib, off, w, h, None, c_all, take, base) == _groups_as_hash_images_wrote_them(off, w, h, c_all, take, base)
    got = _plan(lib, off, w, h, c, 0, take, base)
    assert got == _groups_as_stage_submit_wrote_them(off, w, h, c, take, base)
    return got


def test_one_planner_groups_as_both_loops_did(cpu):
    base = 0x7F0000001000
    assert _hold(cpu, [], [], [], [], [], base) == ([], [])
    assert _hold(cpu, [64], [5], [7], [3], [1], base) == ([(5, 7, 3, 0, 1, 0)], [64, 0])
    assert _hold(cpu, [0, 8, 16], [5, 6, 5], [7, 7, 7], [3, 3, 3], [0, 0, 0], base) == ([], [])
    # seven shapes with repeats, scrambled
    shapes = [(640, 480), (64, 64), (640, 481), (65, 64), (64, 65), (1920, 1080), (1, 1)]
    order = [3, 0, 6, 0, 2, 5, 1, 1, 4, 3, 0, 6, 2, 2, 5, 0, 4, 1]
    w, h = [shapes[k][0] for k in order], [shapes[k][1] for k in order]
    off = (np.arange(len(order)) * 4096).tolist()
    groups, meta = _hold(cpu, off, w, h, [3] * len(order), [1] * len(order), base)
    assert [g[:2] for g in groups] == sorted(shapes) and [g[4] for g in groups] == [order.count(shapes.index(s)) for s in sorted(shapes)]
    take = [k % 5 != 2 for k in range(len(order))]
    _hold(cpu, off, w, h, [3] * len(order), take, base)
    # the same (w, h) with 1, 3 and 4 channels: three groups in the staged form, in channel order
    groups, meta = _plan(cpu, [0, 100, 200, 300, 400], [8] * 5, [9] * 5, [4, 1, 3, 1, 4], 0, [1] * 5, base)
    assert groups == [(8, 9, 1, 0, 2, 0), (8, 9, 3, 4, 1, 0), (8, 9, 4, 6, 2, 0)]
    assert meta == [100, 300, 1, 3, 200, 2, 0, 400, 0, 4]
    assert (groups, meta) == _groups_as_stage_submit_wrote_them([0, 100, 200, 300, 400], [8] * 5, [9] * 5, [4, 1, 3, 1, 4], [1] * 5, base)
    # one image at an address = 2 mod 4: its group alone is misaligned; and a base off by 2 turns it round
    off = [0, 4096, 8194, 12288, 16384]
    w, h = [64, 65, 65, 64, 66], [64] * 5
    groups, _ = _hold(cpu, off, w, h, [3] * 5, [1] * 5, base)
    assert [(g[0], g[5]) for g in groups] == [(64, 0), (65, 1), (66, 0)]
    groups, _ = _hold(cpu, off, w, h, [3] * 5, [1] * 5, base + 2)
    assert [(g[0], g[5]) for g in groups] == [(64, 1), (65, 1), (66, 1)]
    rng = np.random.default_rng(20261019)
    for trial in range(300):
        n = int(rng.integers(0, 60))
        values = rng.choice([1, 3, 64, 65, 640, 2**31 - 1], size=int(rng.integers(1, 5)))
        _hold(cpu, rng.integers(0, 1 << 40, n), rng.choice(values, n), rng.choice(values, n), rng.choice([1, 3, 4], n), rng.integers(0, 4, n) != 0,
              base + int(rng.integers(0, 4)))
