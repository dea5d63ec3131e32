"""The pair plan of the four SSIM pair calls without a GPU: csrc/ke_view_plan.h compiled with the host C++ compiler
(tests/_view_plan_cpu.cpp) into a temporary directory, held against the rules written out a second time here.

The rules (``model`` below, nothing of it read from the header): pair k is box_a[k] of image pair_a[k] as it lies against
orientation orient_b[k] of box_b[k] of image pair_b[k].  A NULL box array, four zeros and (0, 0, w, h) all mean the image as it
lies.  An orientation outside 0..7 is an error for every pair, a box that is empty or leaves its image only where the image
exists; the first one, in the order orientation, side a, side b, ends the call and nothing is planned.  A pair with a missing image
is KE_PAIR_BAD_IMAGE, one whose common size (the smaller width and the smaller height of the two views, a view's sides swapped for
orientation & 4) has a side under 7 KE_PAIR_TOO_SMALL; the others are scored.  Every distinct (image, box, orientation) of a scored
pair is a source, in first-use order: the image itself where nothing is cut or turned, else a plane that is made -- by a crop job
(a box, orientation 0), a turn job (the whole picture turned, as the box (0, 0, w, h)) or a view job (a box turned) -- at the
running offset, which advances by the plane's bytes rounded up to 256.  A common size fits its sources in groups keyed (source
w, source h, made), ascending, each in first-use order.

The calls are the table of the C++ file (at most 8 images and 16 pairs): see the comments there.  Areas 1 and 257 can only be
boxes with a side under 7, so they are too small and take no plane; 255, 256 and 259 show the rounding.  The same source has a
``main`` that plans every call and checks what any plan must satisfy; it is built with AddressSanitizer and UBSan and run as a
program of its own."""
from __future__ import annotations

import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "_view_plan_cpu.cpp")
OK, TOO_SMALL, BAD_IMAGE = 0, 1, 2
CASES = 9


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("view_plan_cpu") / "view_plan_cpu.so")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-O2", "-I", CSRC, SOURCE, "-o", out])
    lib = C.CDLL(out)
    vp, i64 = C.c_void_p, C.c_int64
    lib.vp_cases.restype = i64
    lib.vp_case_name.argtypes, lib.vp_case_name.restype = [i64], C.c_char_p
    lib.vp_case_bad_what.argtypes, lib.vp_case_bad_what.restype = [i64], C.c_char_p
    lib.vp_case_dims.argtypes, lib.vp_case_dims.restype = [i64, vp], None
    lib.vp_case_data.argtypes, lib.vp_case_data.restype = [i64] + [vp] * 8, None
    lib.vp_plan.argtypes = [vp, vp, vp, C.c_int32, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, i64]
    lib.vp_plan.restype = i64
    return lib


def call(cpu, i: int) -> dict:
    """Call i of the table: its arrays, None where the call passes NULL."""
    dims = np.zeros(8, np.int64)
    cpu.vp_case_dims(i, dims.ctypes.data)
    n, has_off, ch, pairs, has_a, has_b, has_o, bad = dims.tolist()
    assert n <= 8 and pairs <= 16
    c = dict(w=np.zeros(n, np.int32), h=np.zeros(n, np.int32), off=np.zeros(n, np.uint64), pa=np.zeros(pairs, np.int64), pb=np.zeros(pairs, np.int64),
             ba=np.zeros((pairs, 4), np.int32), bb=np.zeros((pairs, 4), np.int32), ob=np.zeros(pairs, np.int32))
    cpu.vp_case_data(i, *(c[name].ctypes.data for name in ("w", "h", "off", "pa", "pb", "ba", "bb", "ob")))
    for name, given in (("off", has_off), ("ba", has_a), ("bb", has_b), ("ob", has_o)):
        if not given:
            c[name] = None
    c.update(name=cpu.vp_case_name(i).decode(), channels=ch, bad_pair=bad, bad_what=cpu.vp_case_bad_what(i).decode())
    return c


def planned(cpu, c: dict) -> dict:
    """The header's plan of a call, read back from vp_plan's words."""
    pairs = len(c["pa"])
    ssim, status = np.full(pairs, -2.0), np.full(pairs, -2, np.int32)
    words, error = np.zeros(4096, np.int64), C.create_string_buffer(256)
    addr = lambda a: None if a is None else a.ctypes.data
    used = cpu.vp_plan(addr(c["off"]), addr(c["w"]), addr(c["h"]), c["channels"], len(c["w"]), addr(c["pa"]), addr(c["pb"]), pairs, addr(c["ba"]),
                       addr(c["bb"]), addr(c["ob"]), addr(ssim), addr(status), addr(words), len(words), error, len(error))
    assert used > 0
    it = iter(words[:used].tolist())
    take = lambda count: [next(it) for _ in range(count)]
    p = dict(zip(("bad_pair", "total_bytes", "made_bytes"), take(3)))
    p["srcs"] = [tuple(take(4)) for _ in range(next(it))]
    p["sides"] = [tuple(take(2)) for _ in range(pairs if p["bad_pair"] < 0 else 0)]
    for kind, fields in (("crops", 9), ("turns", 10), ("views", 10)):
        p[kind] = [tuple(take(fields)) for _ in range(next(it))]
    p["sizes"] = {}
    for _ in range(next(it)):
        w, h, count = take(3)
        ks = take(count)
        groups = []
        for _ in range(next(it)):
            gw, gh, made, base, m = take(5)
            groups.append((gw, gh, made, base, take(m)))
        planes = next(it)
        p["sizes"][(w, h)] = dict(pairs=ks, groups=groups, planes=planes, idx=take(2 * count))
    assert next(it, None) is None
    p.update(error=error.value.decode(), ssim=ssim.tolist(), status=status.tolist())
    return p


def model(c: dict) -> dict:
    """The rules of this file's docstring, applied to a call."""
    w, h, ch, n = c["w"].tolist(), c["h"].tolist(), c["channels"], len(c["w"])
    pairs = len(c["pa"])
    exists = lambda i: 0 <= i < n and w[i] > 0 and h[i] > 0

    def box_of(boxes, k, i):                    # None: as it lies
        if boxes is None:
            return None
        b = tuple(boxes[k].tolist())
        return None if b in ((0, 0, 0, 0), (0, 0, w[i], h[i])) else b

    untouched = dict(bad_pair=-1, total_bytes=0, made_bytes=0, srcs=[], sides=[], crops=[], turns=[], views=[], sizes={}, ssim=[-2.0] * pairs,
                     status=[-2] * pairs)
    for k in range(pairs):
        if c["ob"] is not None and not 0 <= c["ob"][k] <= 7:
            return dict(untouched, bad_pair=k, says=("orientation", str(c["ob"][k])))
        for side, images, boxes in (("a", c["pa"], c["ba"]), ("b", c["pb"], c["bb"])):
            i = int(images[k])
            b = box_of(boxes, k, i) if exists(i) else None
            if b is not None and (b[0] < 0 or b[1] < 0 or b[2] <= b[0] or b[3] <= b[1] or b[2] > w[i] or b[3] > h[i]):
                return dict(untouched, bad_pair=k, says=("box_" + side, str(b)))
    offsets, run = [], 0
    for i in range(n):
        offsets.append(int(c["off"][i]) if c["off"] is not None else run)
        run += w[i] * h[i] * ch if w[i] > 0 and h[i] > 0 else 0
    m = dict(untouched, ssim=[], status=[])
    m["total_bytes"] = max([offsets[i] + w[i] * h[i] * ch for i in range(n) if w[i] > 0 and h[i] > 0], default=0)
    source_of, users = {}, {}                   # view -> source; common size -> the pairs scored at it
    for k in range(pairs):
        ia, ib = int(c["pa"][k]), int(c["pb"][k])
        m["ssim"].append(math.nan)
        if not (exists(ia) and exists(ib)):
            m["status"].append(BAD_IMAGE)
            m["sides"].append((-1, -1))
            continue
        views = [(ia, box_of(c["ba"], k, ia), 0), (ib, box_of(c["bb"], k, ib), 0 if c["ob"] is None else int(c["ob"][k]))]
        sizes = []
        for i, b, o in views:
            bw, bh = (w[i], h[i]) if b is None else (b[2] - b[0], b[3] - b[1])
            sizes.append((bh, bw) if o & 4 else (bw, bh))
        common = (min(sizes[0][0], sizes[1][0]), min(sizes[0][1], sizes[1][1]))
        if min(common) < 7:
            m["status"].append(TOO_SMALL)
            m["sides"].append((-1, -1))
            continue
        m["status"].append(OK)
        for (i, b, o), (vw, vh) in zip(views, sizes):
            if (i, b, o) in source_of:
                continue
            source_of[(i, b, o)] = len(m["srcs"])
            if b is None and o == 0:
                m["srcs"].append((0, offsets[i], w[i], h[i]))
                continue
            at = m["made_bytes"]
            m["srcs"].append((1, at, vw, vh))
            x0, y0, x1, y1 = b or (0, 0, w[i], h[i])
            if o == 0:
                m["crops"].append((offsets[i], at, w[i], h[i], ch, x0, y0, x1 - x0, y1 - y0))
            else:
                m["turns" if b is None else "views"].append((offsets[i], at, w[i], h[i], ch, o, x0, y0, x1 - x0, y1 - y0))
            m["made_bytes"] += -(-vw * vh // 256) * 256
        m["sides"].append((source_of[views[0]], source_of[views[1]]))
        users.setdefault(common, []).append(k)
    for common, ks in users.items():
        members = {}                            # group key -> its sources, first use first
        for k in ks:
            for s in m["sides"][k]:
                made, _, sw, sh = m["srcs"][s]
                if s not in members.setdefault((sw, sh, made), []):
                    members[(sw, sh, made)].append(s)
        groups, plane_of, base = [], {}, 0
        for key in sorted(members):
            groups.append(key + (base, members[key]))
            plane_of.update({s: base + j for j, s in enumerate(members[key])})
            base += len(members[key])
        m["sizes"][common] = dict(pairs=ks, groups=groups, planes=base, idx=[plane_of[m["sides"][k][0]] for k in ks] + [plane_of[m["sides"][k][1]] for k in ks])
    return m


def same(got: dict, want: dict) -> None:
    for key in ("bad_pair", "total_bytes", "made_bytes", "srcs", "sides", "crops", "turns", "views", "sizes", "status"):
        assert got[key] == want[key], key
    assert [None if math.isnan(x) else x for x in got["ssim"]] == [None if math.isnan(x) else x for x in want["ssim"]]


@pytest.fixture(scope="module")
def calls(cpu):
    assert cpu.vp_cases() == CASES
    return {c["name"]: c for c in (call(cpu, i) for i in range(CASES))}


def test_the_header_plans_every_call_of_the_table_as_the_rules_do(cpu, calls):
    for c in calls.values():
        got, want = planned(cpu, c), model(c)
        same(got, want)
        assert got["bad_pair"] == c["bad_pair"], c["name"]
        assert list(got["sizes"]) == sorted(got["sizes"]), c["name"]         # the common sizes are walked in ascending order
        if c["bad_pair"] >= 0:                  # the message names the pair, the side and the box, or the orientation
            assert f"pair {c['bad_pair']}:" in got["error"] and c["bad_what"] in got["error"], got["error"]
            assert all(word in got["error"] for word in want["says"]), got["error"]
        else:
            assert got["error"] == ""


def test_the_plain_call(cpu, calls):
    """No boxes, no orientations, offsets NULL: images back to back, the 0 x 10 one taking no bytes; nothing is made."""
    p = planned(cpu, calls["plain"])
    assert p["status"] == [OK, BAD_IMAGE, TOO_SMALL, BAD_IMAGE, BAD_IMAGE, OK, OK, OK, OK]
    assert p["made_bytes"] == 0 and not p["crops"] + p["turns"] + p["views"] and all(s[0] == 0 for s in p["srcs"])
    sizes = [40 * 30, 30 * 40, 0, 6 * 6, 20 * 7, 20 * 7, 300 * 40, 64 * 64]
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]) * 3
    assert p["total_bytes"] == sum(sizes) * 3
    assert [s[1] for s in p["srcs"]] == [starts[i] for i in (0, 1, 4, 5, 6, 7)]           # first use order, each image once
    assert p["sides"][0] == p["sides"][6] == (0, 1) and p["sides"][8] == (1, 0)
    assert sorted(p["sizes"]) == [(20, 7), (30, 30), (64, 40)]


def test_the_three_spellings_of_as_it_lies_are_one(cpu, calls):
    for name in ("as it lies on a", "as it lies on b"):
        c = calls[name]
        got = planned(cpu, c)
        bare = planned(cpu, dict(c, ba=None, bb=None, ob=None))
        same(got, bare)
        assert got["status"] == [OK] * 4 and got["made_bytes"] == 0 and len(got["srcs"]) == 4
    assert [s[1] for s in planned(cpu, calls["as it lies on a"])["srcs"]] == [5000, 100, 9200, 9400]      # the call's own offsets


def test_every_kind_of_view(cpu, calls):
    c = calls["views"]
    p = planned(cpu, c)
    assert p["status"] == [OK] * 6 + [TOO_SMALL] * 3 + [OK] * 3 + [BAD_IMAGE, OK]
    i0, i1, i5, i6 = (int(np.concatenate([[0], np.cumsum(c["w"].astype(np.int64) * c["h"] * 3)])[i]) for i in (0, 1, 5, 6))
    # planes in first-use order: 20x30 crop, 30x40 turned, 30x20 view, 7x20 turned, then 255, 256 and 259 bytes, then 40x30 turned
    starts = [0, 768, 2048, 2816, 3072, 3328, 3584, 4096]
    assert p["made_bytes"] == 4096 + 1280
    assert p["crops"] == [(i1, starts[0], 30, 40, 3, 2, 3, 20, 30), (i6, starts[4], 300, 40, 3, 0, 0, 15, 17), (i6, starts[5], 300, 40, 3, 0, 0, 16, 16)]
    assert p["turns"] == [(i1, starts[1], 30, 40, 3, 3, 0, 0, 30, 40), (i5, starts[3], 20, 7, 3, 4, 0, 0, 20, 7), (i0, starts[7], 40, 30, 3, 1, 0, 0, 40, 30)]
    assert p["views"] == [(i1, starts[2], 30, 40, 3, 5, 2, 3, 20, 30), (i6, starts[6], 300, 40, 3, 6, 0, 0, 7, 37)]
    made = [s for s in p["srcs"] if s[0] == 1]
    assert [(s[2], s[3]) for s in made] == [(20, 30), (30, 40), (30, 20), (7, 20), (15, 17), (16, 16), (37, 7), (40, 30)]
    # the same (image, box, orientation) twice is one source; the image whole and the image boxed are two; a box on side a is the box on side b
    assert p["sides"][2] == p["sides"][3] and p["sides"][4][1] != p["sides"][0][1] and p["sides"][13][0] == p["sides"][0][1]
    assert p["srcs"][p["sides"][4][1]] == (0, i1, 30, 40)
    assert (7, 7) in p["sizes"] and p["sizes"][(7, 7)]["pairs"] == [5]
    # (30, 30): image 0 and image 1 as they lie in one group each, image 1 turned in a third
    assert [g[:3] for g in p["sizes"][(30, 30)]["groups"]] == [(30, 40, 0), (30, 40, 1), (40, 30, 0)]


def test_sanitised_program(tmp_path):
    exe = str(tmp_path / "view_plan_san")
    base = [_cxx(), "-std=c++17", "-Wall", "-O1", "-g", "-DVIEW_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-I", CSRC, SOURCE, "-o", exe]
    if subprocess.run(base + ["-static-libasan"], capture_output=True).returncode != 0:      # (gcc's spelling; clang links it in anyway)
        subprocess.check_call(base)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == f"ok {CASES}" and "runtime error" not in done.stderr
